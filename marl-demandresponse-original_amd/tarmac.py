"""TarMAC-PPO actor and critic (agents/network.py:103-258; learner: agents/tarmac_ppo.py, loop: train_tarmacPPO.py).

``TarMACActor`` keeps the reference's module layout - ``obs2hidden``, ``comm.hidden2key|hidden2value|hidden2query|msg_state2state``,
``comm_hidden2action`` (``hidden2action`` without communication) - so a reference ``actor.pth`` loads with ``load_state_dict``.

Two ways to evaluate the attention of ``TarMAC_Comm.forward``:

``attention="dense"``  the reference's formula in torch on any device: the agents x agents score matrix per env, MaskedSoftmax
                       (utils.py:1353-1358) under the mask of ``make_masks``.  The comparator, the CPU path and the differentiable one.
``attention="band"``   CUDA: in mode "neighbours" the mask is a circular band of c + 1 senders per receiver, so the attention is
                       O(E N c) and runs as ONE HIP kernel per hop (``mdr_tarmac_comm``, include/mdr_policy.h) on keys / values
                       staged in LDS; the five small per-agent MLPs stay library GEMMs into buffers allocated once, the softmax
                       over the two logits and ``Categorical.sample`` are ``mdr_logits_sample``.  Inference only.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as nat

MODES = {"neighbours": 0, "none": 1}      # mdr_tarmac_mode
MAX_HOPS, MAX_KEY, MAX_VALUE, MAX_COMM = 4, 32, 64, 64


def band_offsets(nb_comm: int):
    """The sender offsets of ``make_masks`` (network.py:148-158) after the receiver itself: +1, -1, +2, -2, ..."""
    return [(i + 1) // 2 if i % 2 else -(i // 2) for i in range(1, int(nb_comm) + 1)]


def _mlp(n_in, n_hidden, n_out, act):
    return nn.Sequential(nn.Linear(n_in, n_hidden), act(), nn.Linear(n_hidden, n_out))


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
        if comm_mode not in MODES:
            raise ValueError("tarmac_comm_mode %r: only 'neighbours' and 'none' are covered ('all' and 'random_sample' are not banded)" % (comm_mode,))
        if not 1 <= int(num_hops) <= MAX_HOPS:
            raise ValueError("num_hops must be 1..%d (one Philox word per hop)" % MAX_HOPS)
        if attention not in ("auto", "band", "dense"):
            raise ValueError("attention must be 'auto', 'band' or 'dense'")
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
        if attention == "band":
            self._check_band(None)

    @classmethod
    def from_config(cls, tarmac_ppo_prop: dict, num_obs: int, **kw) -> "TarMACActor":
        """From the reference's ``config_dict["TarMAC_PPO_prop"]`` (agents/tarmac_ppo.py:21-36)."""
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

    def dense_logits(self, obs: torch.Tensor, dead=None) -> torch.Tensor:
        """The reference's forward up to the logits, ``obs`` [E, N, F] in the dtype of the parameters.  ``dead``: the silenced senders,
        bool [E, N] (every hop) or [num_hops, E, N] / a list per hop - required when ``comm_defect_prob > 0`` (the band path draws them
        from Philox; tests hand the same draws over)."""
        x = self.obs2hidden(obs)
        if not self.with_comm:
            return self.hidden2action(x)
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

    def _use_band(self, obs) -> bool:
        if self.attention == "dense":
            return False
        if not obs.is_cuda:
            if self.attention == "band":
                raise ValueError("attention='band' needs the observations and the parameters on the GPU")
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
    def forward(self, obs: torch.Tensor, dead=None, seed: int = 0, step: int = 0, step_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``obs`` [E, N, F] -> probabilities [E, N, 2] (TarMAC_Actor.forward).  Band path: float32 on the GPU, no gradients;
        ``seed`` / ``step`` key the defect draws.  Dense path: differentiable; ``dead`` as in ``dense_logits``."""
        if obs.dim() != 3:
            raise ValueError("TarMAC attends over the agents of an env: obs must be [E, N, F]")
        if dead is None and self._use_band(obs):
            logits = self._band_logits(obs, seed, step, step_dev)
            return self._head(logits, seed, step, step_dev, False, True)[2].view(obs.shape[0], obs.shape[1], 2)
        return F.softmax(self.dense_logits(obs, dead), dim=-1)

    @torch.no_grad()
    def sample(self, obs: torch.Tensor, seed: int, step: int, step_dev: Optional[torch.Tensor] = None, greedy: bool = False,
               dead=None, want_probs: bool = False, action: Optional[torch.Tensor] = None,
               a_prob: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, ...]:
        """``TarmacPPO.select_actions`` (agents/tarmac_ppo.py:83-95) for every env at once: ``obs`` float32 [E, N, F] on the GPU ->
        (action uint8 [E * N], a_prob float32 [E * N][, probs [E * N, 2]]).  The draw is the one of ``FusedActor.sample`` for the same
        (seed, step, agent); ``step_dev`` (device int32) is added to ``step`` inside the kernels.  ``greedy``: the argmax, the first
        maximum on ties.  The dense path (``attention="dense"``, or ``dead`` given) evaluates the reference's formula in torch
        and samples with the same kernel."""
        if not obs.is_cuda:
            raise ValueError("sampling runs on the GPU (mdr_logits_sample); the dense forward() is the CPU path")
        if self.num_action != 2:
            raise ValueError("sampling covers two actions")
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != obs.device):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        if dead is None and self._use_band(obs):
            logits = self._band_logits(obs, seed, step, step_dev)
        else:
            logits = self.dense_logits(obs, dead).reshape(-1, 2).float().contiguous()
        action, a_prob, probs = self._head(logits, seed, step, step_dev, greedy, want_probs, action, a_prob)
        return (action, a_prob, probs) if want_probs else (action, a_prob)


class TarMACCritic(nn.Module):
    """network.py:241-258: the centralised critic, all observations of an env -> one value per agent.  Plain torch."""

    def __init__(self, num_agents: int, num_obs: int, hidden_layer_size: int = 64):
        super().__init__()
        self.critic = nn.Sequential(nn.Linear(num_obs * num_agents, hidden_layer_size), nn.ReLU(),
                                    nn.Linear(hidden_layer_size, hidden_layer_size), nn.ReLU(),
                                    nn.Linear(hidden_layer_size, num_agents))

    def forward(self, obs):
        return self.critic(obs.reshape(obs.shape[0], -1))
