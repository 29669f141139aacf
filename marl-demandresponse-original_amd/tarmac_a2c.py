"""TarMAC A2C on the GPU: the reference's train_tarmac.py (include/mdr_policy.h: mdr_tarmac_a2c_forward / _comm / _grad).

``TarMACA2CPolicy`` is ``MultiAgentPolicy`` (agents/tarmac/model.py:132-266) as ``A2C_ACKTR`` builds it (agents/tarmac/a2c_acktr.py:35-36:
``recurrent_policy=False``, one hop): an actor-critic on a shared trunk whose input is the observation next to the communication
vector of the step before, dense attention over ALL agents of an env (the receiver included), one value per env-step (the mean over
the agents inside the critic).  The submodule layout is the reference's, so its checkpoints load with ``load_state_dict``.

``forward_dense`` is the whole forward in plain torch (differentiable; the CPU path and the comparator).  ``act`` / ``get_value`` run
the act step as HIP kernels: the trunk, the logits and the value (``mdr_tarmac_a2c_forward``), the Philox draw every other actor here
uses (``mdr_logits_sample``), the attention (``mdr_tarmac_a2c_comm``).  ``loss_backward`` is ``A2C_ACKTR.update_multi_agent``'s loss
and ``backward()`` (a2c_acktr.py:59-96) in four launches, exact fp32 (csrc/mdr_tarmac_a2c.hip); ``TarMACA2CLearner`` is the loop with
one Adam over all parameters (or ``optimizer=FusedAdam``: clip + Adam in one launch).  ``evaluate_actions`` discards the new
communication, so the ``base.comm.*`` tensors get no gradient: their ``.grad`` stays as it was (None), and the clip and Adam skip
them, as in the reference.  Nothing on the call path synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _learner as L
from . import _native as nat
from . import graph_update

# the kernels' limits (include/mdr_policy.h: mdr_tarmac_a2c_*)
MAX_OBS, MAX_COMM, MAX_STATE, MAX_KEY, MAX_AGENTS = 128, 32, 128, 16, 64
# backend="auto" and the default act path follow profiles/tarmac_a2c_README.md: the kernels where they measured faster than the torch
# comparator by more than its run-to-run spread, torch elsewhere - counted in agent rows (env-steps x agents), what every pass of the
# kernels walks.  Update step: 2.2x to 4.3x faster from 640 rows (32 env-steps of 20 agents) to 5120 (256 x 20), and at 50 x 64; at
# 50 x 128 (6400 rows) the lead of 1.6x was inside the comparator's spread in one of two runs, at 512 x 20 the bare backward loses,
# at 4096 x 20 the kernels take 5x as long (the weight pass walks all rows in one wave per block).  Act step: 3.3x faster from 1 to
# 64 envs of 20 agents, 2.9x at 256, 1.17x at 1024 (20480 rows), 0.36x at 4096.
AUTO_MIN_AGENT_ROWS = 1
AUTO_MAX_AGENT_ROWS = 5120
ACT_AUTO_MAX_AGENT_ROWS = 20480


class MeanAll(nn.Module):
    """agents/tarmac/model.py:14-21."""

    def __init__(self, dim: int, keepdim: bool = False):
        super().__init__()
        self.dim, self.keepdim = dim, keepdim

    def forward(self, x):
        return x.mean(dim=self.dim, keepdim=self.keepdim)


class CommAttention(nn.Module):
    """model.py:50-129 without the (P N)^2 mask: envs are the batch dimension."""

    def __init__(self, state_size: int, comm_size: int, key_size: int, num_hops: int):
        super().__init__()
        self.state_size, self.comm_size, self.key_size, self.num_hops = state_size, comm_size, key_size, num_hops
        self.msg2nextstate = nn.Sequential(nn.Linear(state_size + comm_size, state_size), nn.LeakyReLU())
        self.state2query = nn.Linear(state_size, key_size)
        self.state2key = nn.Linear(state_size, key_size)
        self.state2value = nn.Linear(state_size, comm_size)

    def forward(self, states):
        """``states`` [E, N, S] -> (attention of the last hop [E, N, N], comm [E, N, C])."""
        attn = comm = None
        for hop in range(self.num_hops):
            if hop > 0:
                states = self.msg2nextstate(torch.cat([comm, states], dim=2))      # comm first (model.py:124)
            q, k, v = self.state2query(states), self.state2key(states), self.state2value(states)
            scores = torch.matmul(q, k.transpose(1, 2)) / math.sqrt(self.comm_size)      # sqrt(comm_size), model.py:115-116
            attn = F.softmax(scores, dim=-1)
            comm = torch.matmul(attn, v)
        return attn, comm


class _Base(nn.Module):
    def __init__(self, nb_obs, state_size, comm_size, key_size, num_hops):
        super().__init__()
        self.common = nn.Sequential(nn.Linear(nb_obs + comm_size, state_size), nn.LeakyReLU(), nn.Linear(state_size, state_size))
        self.critic = nn.Sequential(nn.Linear(state_size, state_size), MeanAll(dim=1), nn.LeakyReLU(), nn.Linear(state_size, 1))
        self.comm = CommAttention(state_size, comm_size, key_size, num_hops)


class _Categorical(nn.Module):
    """agents/tarmac/distributions.py:31-44: one bias-free Linear, orthogonal at gain 0.01."""

    def __init__(self, num_inputs: int, num_outputs: int):
        super().__init__()
        self.linear = nn.Linear(num_inputs, num_outputs, bias=False)
        nn.init.orthogonal_(self.linear.weight, gain=0.01)


class TarMACA2CPolicy(nn.Module):
    """``MultiAgentPolicy`` of train_tarmac.py.  state_dict keys: ``base.common.{0,2}``, ``base.critic.{0,3}``,
    ``base.comm.msg2nextstate.0``, ``base.comm.state2{query,key,value}``, ``dist.linear.weight``."""

    def __init__(self, nb_obs: int, state_size: int = 128, comm_size: int = 32, key_size: int = 16, num_hops: int = 1,
                 recurrent_policy: bool = False):
        super().__init__()
        if recurrent_policy:
            raise ValueError("recurrent_policy=True is not covered: A2C_ACKTR builds MultiAgentPolicy with recurrent_policy=False whatever "
                             "the config says (agents/tarmac/a2c_acktr.py:35)")
        if num_hops < 1:
            raise ValueError("num_hops must be at least 1")
        self.nb_obs, self.state_size, self.comm_size, self.key_size, self.num_hops = int(nb_obs), int(state_size), int(comm_size), int(key_size), int(num_hops)
        self.base = _Base(self.nb_obs, self.state_size, self.comm_size, self.key_size, self.num_hops)
        self.dist = _Categorical(self.state_size, 2)

    @classmethod
    def from_config(cls, tarmac_prop: dict, nb_obs: int) -> "TarMACA2CPolicy":
        """From the reference's ``config_dict["TarMAC_prop"]``: state_size and communication_size; recurrent_policy and comm_num_hops
        are overridden by A2C_ACKTR.__init__ (a2c_acktr.py:35-36) and not read."""
        return cls(nb_obs, state_size=tarmac_prop["state_size"], comm_size=tarmac_prop["communication_size"])

    # ------------------------------------------------------------------------------------------------------------------ torch
    def forward_dense(self, obs: torch.Tensor, comm_in: torch.Tensor):
        """MultiAgentBase.forward + dist (model.py:244-266) in plain torch, a batched matmul over the envs: ``obs`` [E, N, F],
        ``comm_in`` [E, N, C] -> (value [E], logits [E, N, 2], x [E, N, S], comm_out [E, N, C], attn [E, N, N]).  Differentiable."""
        if obs.dim() != 3 or comm_in.dim() != 3 or obs.shape[:2] != comm_in.shape[:2]:
            raise ValueError("obs must be [E, N, F] and comm_in [E, N, C]")
        x = self.base.common(torch.cat([obs, comm_in], dim=2))
        attn, comm_out = self.base.comm(x)
        value = self.base.critic(x).squeeze(-1)
        return value, self.dist.linear(x), x, comm_out, attn

    # ---------------------------------------------------------------------------------------------------------------- kernels
    def _act_kernels(self, nb_envs: int, nb_agents: int) -> bool:
        return nb_envs * nb_agents <= ACT_AUTO_MAX_AGENT_ROWS and _refusal(self, nb_agents) is None

    def _check_act(self, obs, comm_in, what):
        if obs.dim() != 3 or obs.shape[2] != self.nb_obs or obs.dtype != torch.float32 or not obs.is_cuda or not obs.is_contiguous():
            raise ValueError("%s: obs must be a contiguous float32 [E, N, %d] tensor on the GPU (forward_dense is the CPU path)" % (what, self.nb_obs))
        E, N = int(obs.shape[0]), int(obs.shape[1])
        if (comm_in.dim() != 3 or tuple(comm_in.shape) != (E, N, self.comm_size) or comm_in.dtype != torch.float32 or comm_in.device != obs.device
                or comm_in.stride(2) != 1 or comm_in.stride(1) < self.comm_size or (E > 1 and comm_in.stride(0) != N * comm_in.stride(1))):
            raise ValueError("%s: comm_in must be a float32 [E, N, %d] tensor on the device with one row stride over all agents" % (what, self.comm_size))
        return E, N

    def forward_kernels(self, obs: torch.Tensor, comm_in: torch.Tensor, want_x: bool = True):
        """``mdr_tarmac_a2c_forward``: (logits [E N, 2], value [E], x [E N, S] or None) - bit for bit what ``loss_backward`` forms on
        the same rows.  ValueError for a policy the kernels refuse."""
        E, N = self._check_act(obs, comm_in, "forward_kernels")
        why = _refusal(self, N)
        if why:
            raise ValueError("forward_kernels: " + why)
        dev = obs.device
        lib = nat.load()
        desc = _desc(self)
        logits = torch.empty((E * N, 2), dtype=torch.float32, device=dev)
        value = torch.empty(E, dtype=torch.float32, device=dev)
        x = torch.empty((E * N, self.state_size), dtype=torch.float32, device=dev) if want_x else None
        ws = None if want_x else L.workspace(dev, int(lib.mdr_tarmac_a2c_workspace_bytes(C.byref(desc), E, N, 0)))
        with torch.cuda.device(dev):
            rc = lib.mdr_tarmac_a2c_forward(C.byref(desc), L.ptr(obs), self.nb_obs, L.ptr(comm_in), int(comm_in.stride(1)), None, E, N, 0, L.ptr(ws),
                                            L.ptr(logits), L.ptr(value), L.ptr(x), L.stream(dev))
        nat.check(lib, None, rc, "mdr_tarmac_a2c_forward")
        return logits, value, x

    def comm_kernel(self, x: torch.Tensor, nb_envs: int, nb_agents: int, out: Optional[torch.Tensor] = None, want_attn: bool = False):
        """``mdr_tarmac_a2c_comm``: ``x`` [E N, S] -> comm_out [E, N, C] (into ``out``: float32 [E, N, C] with unit inner stride and one
        row stride >= C over all agents) [and attn [E, N, N]]."""
        E, N, Cc = int(nb_envs), int(nb_agents), self.comm_size
        dev = x.device
        if out is None:
            out = torch.empty((E, N, Cc), dtype=torch.float32, device=dev)
        elif (tuple(out.shape) != (E, N, Cc) or out.dtype != torch.float32 or out.device != dev or out.stride(2) != 1 or out.stride(1) < Cc
              or (E > 1 and out.stride(0) != N * out.stride(1))):
            raise ValueError("comm_kernel: out must be a float32 [E, N, %d] tensor on the device with one row stride over all agents" % Cc)
        if x.dtype != torch.float32 or not x.is_contiguous() or x.numel() != E * N * self.state_size:
            raise ValueError("comm_kernel: x must be a contiguous float32 [E N, S] tensor")
        attn = torch.empty((E, N, N), dtype=torch.float32, device=dev) if want_attn else None
        lib = nat.load()
        desc = _desc(self)
        with torch.cuda.device(dev):
            rc = lib.mdr_tarmac_a2c_comm(C.byref(desc), L.ptr(x), E, N, 0, L.ptr(out), int(out.stride(1)), L.ptr(attn), L.stream(dev))
        nat.check(lib, None, rc, "mdr_tarmac_a2c_comm")
        return (out, attn) if want_attn else out

    @torch.no_grad()
    def act(self, obs: torch.Tensor, comm_in: torch.Tensor, seed: int, step: int, step_dev: Optional[torch.Tensor] = None,
            greedy: bool = False, action: Optional[torch.Tensor] = None, a_prob: Optional[torch.Tensor] = None,
            comm_out: Optional[torch.Tensor] = None, kernels: Optional[bool] = None):
        """``MultiAgentPolicy.act`` (model.py:169-178) for every env at once: ``obs`` float32 [E, N, F], ``comm_in`` [E, N, C] (the
        ``comm_out`` of the step before; zeros after a reset) on the GPU -> (action uint8 [E N], a_prob float32 [E N] - the probability
        of the taken action -, value [E], comm_out [E, N, C]).  The draw is ``mdr_logits_sample``'s: the Philox draw of every other actor
        for the same (seed, step, agent); ``step_dev`` (device int32) is added to ``step`` inside the kernel; ``greedy``: the argmax.
        ``kernels``: None - the HIP kernels wherever they take the policy (``supported``) and measured faster (at most
        ``ACT_AUTO_MAX_AGENT_ROWS`` agents in all, profiles/tarmac_a2c_README.md), ``forward_dense`` otherwise (also: more than one
        hop, sizes outside the limits); True - required (ValueError where refused); False - torch."""
        E, N = self._check_act(obs, comm_in, "act")
        dev = obs.device
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != dev):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        if kernels is None:
            kernels = self._act_kernels(E, N)
        if kernels:
            logits, value, x = self.forward_kernels(obs, comm_in)
        else:
            value, logits, _, dense_comm, _ = self.forward_dense(obs, comm_in)
            logits = logits.reshape(E * N, 2).contiguous()
        if action is None:
            action = torch.empty(E * N, dtype=torch.uint8, device=dev)
        if a_prob is None:
            a_prob = torch.empty(E * N, dtype=torch.float32, device=dev)
        lib = nat.load()
        with torch.cuda.device(dev):
            rc = lib.mdr_logits_sample(L.ptr(logits), 2, E * N, C.c_uint64(int(seed) & (2 ** 64 - 1)), C.c_uint64(int(step) & (2 ** 64 - 1)),
                                       L.ptr(step_dev), int(bool(greedy)), L.ptr(action), L.ptr(a_prob), None, L.stream(dev))
        nat.check(lib, None, rc, "mdr_logits_sample")
        if kernels:
            comm_out = self.comm_kernel(x, E, N, out=comm_out)
        elif comm_out is None:
            comm_out = dense_comm
        else:
            comm_out.copy_(dense_comm)
        return action, a_prob, value, comm_out

    @torch.no_grad()
    def get_value(self, obs: torch.Tensor, comm_in: torch.Tensor) -> torch.Tensor:
        """``MultiAgentPolicy.get_value`` (model.py:180-183): [E] - one value per env."""
        if obs.is_cuda and _refusal(self, int(obs.shape[1]) if obs.dim() == 3 else None) is None:
            return self.forward_kernels(obs, comm_in, want_x=False)[1]
        return self.forward_dense(obs, comm_in)[0]


def _reached(policy) -> List[torch.Tensor]:
    """The nine tensors an update reaches, in ``parameters()`` order - the order of the flat gradient."""
    b = policy.base
    return [b.common[0].weight, b.common[0].bias, b.common[2].weight, b.common[2].bias, b.critic[0].weight, b.critic[0].bias,
            b.critic[3].weight, b.critic[3].bias, policy.dist.linear.weight]


def _kernel_params(policy) -> List[torch.Tensor]:
    """The fifteen tensors of ``mdr_tarmac_a2c_net_t``, in its order."""
    c = policy.base.comm
    return _reached(policy)[:8] + [c.state2query.weight, c.state2query.bias, c.state2key.weight, c.state2key.bias, c.state2value.weight,
                                   c.state2value.bias, policy.dist.linear.weight]


def _refusal(policy, nb_agents: Optional[int] = None) -> Optional[str]:
    """Why the kernels do not take ``policy`` (None: they do)."""
    if not isinstance(policy, TarMACA2CPolicy):
        return "the kernels cover a TarMACA2CPolicy"
    if policy.num_hops != 1:
        return "num_hops = %d: the kernels cover one hop (forward_dense covers more)" % policy.num_hops
    F_, Cc, S, K = policy.nb_obs, policy.comm_size, policy.state_size, policy.key_size
    if not 1 <= F_ <= MAX_OBS:
        return "nb_obs = %d: the kernels cover 1 to %d features" % (F_, MAX_OBS)
    if S < 4 or S % 4 or S > MAX_STATE:
        return "state_size = %d: the kernels cover a multiple of 4 <= %d" % (S, MAX_STATE)
    if Cc < 4 or Cc % 4 or Cc > MAX_COMM or K < 4 or K % 4 or K > MAX_KEY:
        return "comm_size = %d, key_size = %d: the kernels cover multiples of 4 <= %d and <= %d" % (Cc, K, MAX_COMM, MAX_KEY)
    if nb_agents is not None and not 1 <= nb_agents <= MAX_AGENTS:
        return "%d agents per env: the kernels cover 1 to %d" % (nb_agents, MAX_AGENTS)
    for p in _kernel_params(policy):
        if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
            return "parameters must be contiguous float32 tensors on the GPU"
    return None


def supported(policy) -> bool:
    """Do the kernels take this policy?  A one-hop ``TarMACA2CPolicy`` with nb_obs <= 128, state_size a multiple of 4 <= 128,
    comm_size a multiple of 4 <= 32, key_size a multiple of 4 <= 16, float32 on the GPU (and at most 64 agents per env)."""
    return _refusal(policy) is None


def _desc(policy) -> nat.MdrTarmacA2CNet:
    ptr = [C.c_void_p(p.data_ptr()) for p in _kernel_params(policy)]
    return nat.MdrTarmacA2CNet(C.sizeof(nat.MdrTarmacA2CNet), policy.nb_obs, policy.comm_size, policy.state_size, policy.key_size, *ptr)


def _rows(t, width, what, name, dev):
    """``t`` float32 [M, N, width] with unit inner stride and one row stride >= width over all agents -> (M, N, ld)."""
    if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.shape[2] != width or t.dtype != torch.float32 or t.device != dev:
        raise ValueError("%s: %s must be a float32 [M, N, %d] tensor on %s" % (what, name, width, dev))
    M, N = int(t.shape[0]), int(t.shape[1])
    ld = int(t.stride(1)) if N > 1 else (int(t.stride(0)) if M > 1 else width)
    if (width > 1 and t.stride(2) != 1) or ld < width or (M > 1 and N > 1 and t.stride(0) != N * ld):
        raise ValueError("%s: %s rows need unit inner stride and one row stride >= %d over all agents" % (what, name, width))
    return M, N, ld


def loss_backward(policy, obs: torch.Tensor, comm: torch.Tensor, action: torch.Tensor, ret: torch.Tensor, value_loss_coef: float = 0.5,
                  entropy_coef: float = 0.01, index: Optional[torch.Tensor] = None, want_value: bool = False, max_workgroups: int = 0):
    """The loss of a2c_acktr.py:61-96 and ``backward()``: fills ``p.grad`` of the nine parameters an update reaches (views of one flat
    buffer kept with the module, whatever ``.grad`` was there before - a tensor that was there is overwritten with the gradient and then
    replaced by the view) and leaves the ``.grad`` of the ``base.comm.*`` tensors as
    it was.  -> (value_loss, action_loss, entropy) as 0-dim device tensors [, value [B], advantage [B, N]].  ``obs`` float32
    [M, N, F], ``comm`` float32 [M, N, C] (the stored comm_in), ``action`` int64 [M, N], ``ret`` float32 [M, N]: the stored env-steps,
    read in place through ``index`` (int64 [B] on the device; None: every env-step in order, B = M)."""
    what = "tarmac_a2c.loss_backward"
    if not isinstance(obs, torch.Tensor) or obs.dim() != 3:
        raise ValueError("%s: obs must be [M, N, F]" % what)
    why = _refusal(policy, int(obs.shape[1]))
    if why:
        raise ValueError("%s: %s" % (what, why))
    dev = policy.dist.linear.weight.device
    M, N, ld_obs = _rows(obs, policy.nb_obs, what, "obs", dev)
    Mc, Nc, ld_comm = _rows(comm, policy.comm_size, what, "comm", dev)
    if (Mc, Nc) != (M, N):
        raise ValueError("%s: comm must hold the same [M, N] env-steps as obs" % what)
    L.check_index(index, dev, what)
    B = int(index.shape[0]) if index is not None else M
    L.whole(action, torch.int64, M * N, dev, what, "action")
    L.whole(ret, torch.float32, M * N, dev, what, "ret")
    desc = _desc(policy)
    floats, nbytes = _grad_sizes(desc, B, N, max_workgroups, what)
    flat = L.flat_grad(policy, floats, dev)
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    value = torch.empty(B, dtype=torch.float32, device=dev) if want_value else None
    advantage = torch.empty((B, N), dtype=torch.float32, device=dev) if want_value else None
    with torch.cuda.device(dev):
        _grad_launch(desc, obs, ld_obs, comm, ld_comm, action, ret, index, B, N, L.workspace(dev, nbytes), flat, losses, value, advantage,
                     L.stream(dev), value_loss_coef, entropy_coef, max_workgroups)
    L.publish(_reached(policy), flat, L.REPLACE)      # whoever holds a tensor that was there sees the new gradient too
    out = (losses[0], losses[1], losses[2])
    return out + (value, advantage) if want_value else out


def _grad_sizes(desc, B: int, N: int, max_workgroups: int = 0, what: str = "tarmac_a2c") -> Tuple[int, int]:
    """(floats of the flat gradient, bytes of workspace) of an ``mdr_tarmac_a2c_grad`` call over ``B`` env-steps of ``N`` agents."""
    lib = nat.load()
    return (int(lib.mdr_tarmac_a2c_grad_floats(C.byref(desc))),
            L.sized(lib.mdr_tarmac_a2c_workspace_bytes(C.byref(desc), B, N, max_workgroups), what, "mdr_tarmac_a2c_workspace_bytes"))


def _grad_launch(desc, obs, ld_obs, comm, ld_comm, action, ret, index, B, N, workspace, flat, losses, value, advantage, stream,
                 value_loss_coef: float, entropy_coef: float, max_workgroups: int = 0) -> None:
    """mdr_tarmac_a2c_grad on checked tensors and caller-owned buffers, under the device of ``obs``: the eager call and the captured one."""
    lib = nat.load()
    rc = lib.mdr_tarmac_a2c_grad(C.byref(desc), L.ptr(obs), ld_obs, L.ptr(comm), ld_comm, L.ptr(action), L.ptr(ret), L.ptr(index), B, N,
                                 C.c_float(value_loss_coef), C.c_float(entropy_coef), max_workgroups, L.ptr(workspace), L.ptr(flat), L.ptr(losses),
                                 L.ptr(value), L.ptr(advantage), stream)
    nat.check(lib, None, rc, "mdr_tarmac_a2c_grad")


def dense_losses(policy, obs, comm, action, ret):
    """a2c_acktr.py:61-92 on ``forward_dense`` under autograd: ``obs`` [B, N, F], ``comm`` [B, N, C], ``action`` int64 [B, N], ``ret``
    [B, N] -> (value_loss, action_loss, entropy), differentiable."""
    value, logits, _, _, _ = policy.forward_dense(obs, comm)
    logp = F.log_softmax(logits, dim=-1)
    advantage = ret - value[:, None]
    value_loss = advantage.pow(2).mean()
    action_loss = -(advantage.detach() * logp.gather(2, action.unsqueeze(2)).squeeze(2)).mean()
    entropy = -(logp.exp() * logp).sum(dim=-1).mean()
    return value_loss, action_loss, entropy


class TarMACA2CLearner:
    """``A2C_ACKTR.update_multi_agent`` (agents/tarmac/a2c_acktr.py:59-107) on the dict ``collect_tarmac_a2c_rollout`` returns: per
    minibatch loss = value_loss_coef value_loss + action_loss - entropy_coef entropy, ``clip_grad_norm_`` over all parameters, ONE Adam
    step over all parameters (only ``lr`` is passed: torch's default eps).

    ``backend="hip"``: ``loss_backward`` (ValueError for a policy the kernels refuse); ``"torch"``: autograd on ``forward_dense`` - the
    comparator, the CPU path and the path for more than one hop; ``"auto"``: the kernels where ``supported(policy)`` holds and the
    minibatch has ``AUTO_MIN_AGENT_ROWS`` to ``AUTO_MAX_AGENT_ROWS`` agent rows - env-steps x agents - (where they measured
    faster, profiles/tarmac_a2c_README.md), torch otherwise.  ``optimizer=FusedAdam``: clip + Adam in one launch; parameters whose ``grad`` is
    None (``base.comm.*``) are skipped, as torch's Adam skips them.

    ``sampler="philox"``: the minibatch indices from csrc/mdr_minibatch.hip by (seed, epoch) instead of a ``torch.Generator`` (default
    ``"torch"``; ``"philox"`` under ``graph=True``).  ``graph=True``: every epoch of an update replayed from one captured graph per
    batch shape (graph_update.TarMACA2CUpdateGraph), the bits of the eager ``sampler="philox"`` update; it needs the kernels,
    ``optimizer=FusedAdam`` and the philox sampler.  ``graph_max_minibatches`` bounds the minibatches (of env-steps) per epoch."""

    def __init__(self, policy, lr: float = 7e-4, value_loss_coef: float = 0.5, entropy_coef: float = 0.01, max_grad_norm: float = 0.5,
                 nb_updates: int = 10, batch_size: int = 128, backend: str = "auto", optimizer=torch.optim.Adam,
                 sampler: Optional[str] = None, graph: bool = False, graph_max_minibatches: int = 1024):
        L.check_backend(backend)
        sampler = L.check_sampler(sampler, graph)
        if backend == "hip":
            L.require(_refusal(policy), "TarMACA2CLearner")
        self.policy = policy
        self.value_loss_coef, self.entropy_coef, self.max_grad_norm = float(value_loss_coef), float(entropy_coef), float(max_grad_norm)
        self.nb_updates, self.batch_size, self.backend = int(nb_updates), int(batch_size), backend
        self.optimizer = optimizer(policy.parameters(), lr)
        self.training_step = 0
        self.sampler, self.graph, self.graph_max_minibatches = sampler, bool(graph), int(graph_max_minibatches)
        self.graph_captures = 0
        self._graphs: Dict[tuple, object] = {}
        if self.graph:
            # the agents per env come with the batch: "auto" is held to its window again at every update (graph_update.tarmac_a2c_update)
            takes = _refusal(policy) is None if backend == "auto" else backend == "hip"
            why = graph_update.refusal(backend, sampler, (self.optimizer,), takes)
            if not why and backend == "auto":
                why = _refusal(policy)
            if why:
                raise ValueError("TarMACA2CLearner(graph=True): %s" % why)

    @classmethod
    def from_config(cls, tarmac_prop: dict, policy, backend: str = "auto", optimizer=torch.optim.Adam, sampler: Optional[str] = None,
                    graph: bool = False, graph_max_minibatches: int = 1024) -> "TarMACA2CLearner":
        """From the reference's ``config_dict["TarMAC_prop"]`` (a2c_acktr.py:17-32); tarmac_eps and tarmac_alpha belong to the
        RMSprop line the reference has commented out and are not read."""
        p = tarmac_prop
        return cls(policy, lr=p["tarmac_lr"], value_loss_coef=p["value_loss_coef"], entropy_coef=p["entropy_coef"],
                   max_grad_norm=p["tarmac_max_grad_norm"], nb_updates=p["nb_tarmac_updates"], batch_size=p["tarmac_batch_size"],
                   backend=backend, optimizer=optimizer, sampler=sampler, graph=graph, graph_max_minibatches=graph_max_minibatches)

    def uses_kernels(self, nb_env_steps: int, nb_agents: int) -> bool:
        if self.backend == "auto":
            return AUTO_MIN_AGENT_ROWS <= nb_env_steps * nb_agents <= AUTO_MAX_AGENT_ROWS and _refusal(self.policy, nb_agents) is None
        return self.backend == "hip"

    def minibatches(self, nb_env_steps: int, seed: int, epoch: int) -> List[torch.Tensor]:
        """The index tensors of one epoch over the stored env-steps (``_learner.minibatches`` under this learner's sampler)."""
        return L.minibatches(next(self.policy.parameters()).device, nb_env_steps, self.batch_size, self.sampler, seed, epoch)

    def _capture(self, shape, nb_agents: int):
        """Capture the graph of one epoch over a batch of ``shape`` = (T, A, F) - A = E N agents per step, N = ``nb_agents`` - without
        replaying it; parameters, moments and every counter are what they were."""
        T, A, F = (int(x) for x in shape)
        g = graph_update.TarMACA2CUpdateGraph(self, T, A, int(nb_agents), F)
        self._graphs[(T, A, int(nb_agents), F, self.nb_updates, self.batch_size)] = g
        self.graph_captures += 1
        return g

    def step_minibatch(self, obs, comm, action, ret, index) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One minibatch of a2c_acktr.py:61-107 on the whole buffers ``obs`` [M, N, F], ``comm`` [M, N, C], ``action``, ``ret`` [M, N];
        ``index`` picks the env-steps.  -> (value_loss, action_loss, entropy)."""
        if self.uses_kernels(int(index.shape[0]), int(obs.shape[1])):      # the kernels overwrite the gradient: no zero_grad()
            value_loss, action_loss, entropy = loss_backward(self.policy, obs, comm, action, ret, self.value_loss_coef, self.entropy_coef,
                                                             index=index)
        else:
            value_loss, action_loss, entropy = dense_losses(self.policy, obs[index], comm[index], action[index], ret[index])
            self.optimizer.zero_grad()
            (value_loss * self.value_loss_coef + action_loss - entropy * self.entropy_coef).backward()
            value_loss, action_loss, entropy = value_loss.detach(), action_loss.detach(), entropy.detach()
        L.clip_and_step(self.optimizer, self.policy.parameters(), self.max_grad_norm)
        self.training_step += 1
        return value_loss, action_loss, entropy

    def update(self, batch: Dict[str, torch.Tensor], seed: int = 0, nb_agents: Optional[int] = None):
        """``nb_updates`` epochs over ``batch`` (``state`` [T+1, E*N, F], ``comm`` [T+1, E*N, C], ``action``, ``return`` [T, E*N],
        ``value`` [T+1, E] - which gives E): the T E stored env-steps are ``state[:-1]`` and ``comm[:-1]`` viewed as [T E, N, .] and read
        in place.  -> (mean value_loss, mean action_loss, mean entropy - device tensors -, number of minibatches).  ``graph=True``: the
        same launches replayed from a captured graph, the same bits as the eager ``sampler="philox"`` update."""
        if self.graph:
            done = graph_update.tarmac_a2c_update(self, batch, seed, nb_agents)
            if done is not None:      # None: an empty batch, nothing to replay
                return done
        states, comms = batch["state"], batch["comm"]
        T = states.shape[0] - 1
        N = int(nb_agents) if nb_agents is not None else states.shape[1] // int(batch["value"].shape[1])
        if states.shape[1] % N:
            raise ValueError("TarMACA2CLearner.update: %d agents per step are no whole number of envs of %d agents" % (states.shape[1], N))
        obs = states[:T].reshape(-1, N, states.shape[-1])      # views: the first T slabs of contiguous buffers
        comm = comms[:T].reshape(-1, N, comms.shape[-1])
        action = batch["action"].reshape(-1, N)
        ret = batch["return"].reshape(-1, N)
        n = obs.shape[0]
        sums = torch.zeros(3, dtype=torch.float32, device=obs.device)
        count = 0
        for epoch in range(self.nb_updates):
            for index in self.minibatches(n, seed, epoch):
                v, a, e = self.step_minibatch(obs, comm, action, ret, index)
                sums += torch.stack([v, a, e])
                count += 1
        sums = sums / max(count, 1)
        return sums[0], sums[1], sums[2], count
