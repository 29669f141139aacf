"""DQN's and DDQN's update step on the GPU (include/mdr_policy.h: mdr_dqn_target, mdr_dqn_grad).

The other half of the reference's train_dqn.py: ``DQN.update`` (agents/dqn.py:84-112) and ``DDQN.update`` (:119-146) on the transitions
``rollout.collect_dqn_transitions`` leaves on the device.  Per update the reference samples a minibatch from its replay buffer,
evaluates the target net on the next states (DDQN: the policy net too), forms ``reward + gamma * next_q``, evaluates the policy net on
the states, takes ``nn.SmoothL1Loss``, calls ``backward()``, clamps every gradient element to [-1, 1], takes an Adam step and blends
the target net towards the policy net.  Here the target is ONE forward-only HIP kernel on the matrix cores (two for DDQN) and forward,
Huber loss, backward and the clamp are one more plus its reduction: ``td_target`` / ``q_loss_backward``.  torch keeps the optimiser
and the blend by default; ``optimizer=FusedAdam`` (optim.py) makes them one more launch.  ``DeviceReplayBuffer`` is the reference's ``ReplayBuffer`` as preallocated device tensors the kernels read in place
through the sampled indices, ``DQNLearner`` the update, ``train_dqn`` the loop.  Nothing on the call path synchronises with the host.

Two places leave the reference's text on purpose:

* ``DDQN.update`` adds ``reward`` [B, 1] to ``next_q_values.unsqueeze(1)`` [B, 1, 1], which broadcasts the target to [B, B, 1] - every
  row's Q-value is regressed on every other row's target (agents/dqn.py:132-135).  Both backends build the per-row target
  ``reward_i + gamma * Q_target(s'_i, argmax_a Q_policy(s'_i, a))`` that line evidently means.
* ``DDQN.update`` never calls ``update_target_network()``, so its target net stays at its initial weights for ever.  ``DQNLearner``
  soft-updates in both modes; ``soft_update=False`` reproduces the omission.
"""
from __future__ import annotations

import ctypes as C
from functools import partial
from typing import Dict, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _learner as L
from . import _native as nat
from . import graph_update
from .optim import FusedAdam
from .ppo import refusal

# backend="auto": the kernels from this many minibatch rows on (profiles/dqn_update_README.md: where they measured faster than autograd)
AUTO_MIN_ROWS = 1
# the same for wide=True, 65..128 input features (profiles/wide_update_README.md)
AUTO_MIN_ROWS_WIDE = 1


class QNetworkMLP(nn.Module):
    """agents/network.py:58-77 (``DQN_network``) - the Linear/ReLU stack of the PPO actor with raw Q-values for a head; state_dict keys
    ``fc.<i>.weight|bias``, so the ``actor.pth`` of ``DQN.save()`` loads with ``load_state_dict``."""

    def __init__(self, num_state: int, num_action: int = 2, layers: Sequence[int] = (100, 100)):
        super().__init__()
        dims = [num_state] + [int(x) for x in layers]
        self.layers = list(layers)
        self.fc = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
        self.fc.append(nn.Linear(dims[-1], num_action))

    def forward(self, x):
        for lin in self.fc[:-1]:
            x = F.relu(lin(x))
        return self.fc[-1](x)


def supported(net, wide: bool = False) -> bool:
    """Do the kernels take this Q-network?  Two hidden layers, F <= 64 input features, at most 128 hidden units, 2 actions, float32
    on the GPU.  ``wide=True``: the wide entry points, F <= 128 where the LDS layout fits (hidden 100-100: every F; 128-128: F <= 100)."""
    return refusal(net, 2, wide=wide) is None


def _target_launch(tdesc, pdesc, next_state, ld, reward, index, B, y, next_q, next_action, stream, gamma, max_workgroups=0, wide=False) -> None:
    """mdr_dqn_target[_wide] on checked tensors (``pdesc`` None: DQN), under the device of ``next_state``: the eager call and the
    captured one."""
    lib = nat.load()
    call, name = L.fn(lib, "mdr_dqn_target", wide)
    nat.check(lib, None, call(C.byref(tdesc), C.byref(pdesc) if pdesc is not None else None, L.ptr(next_state), ld, L.ptr(index), B, L.ptr(reward),
                              C.c_float(gamma), max_workgroups, L.ptr(y), L.ptr(next_q), L.ptr(next_action), stream), name)


def _grad_launch(desc, state, ld, action, y, index, B, workspace, flat, loss, q, stream, grad_clamp, max_workgroups=0, wide=False) -> None:
    """mdr_dqn_grad[_wide] on checked tensors: the eager call and the captured one."""
    lib = nat.load()
    call, name = L.fn(lib, "mdr_dqn_grad", wide)
    nat.check(lib, None, call(C.byref(desc), L.ptr(state), ld, L.ptr(index), B, L.ptr(action), L.ptr(y), C.c_float(grad_clamp), max_workgroups,
                              L.ptr(workspace), L.ptr(flat), L.ptr(loss), L.ptr(q), stream), name)


def td_target(target_net, next_state: torch.Tensor, reward: torch.Tensor, gamma: float, index: Optional[torch.Tensor] = None,
              policy_net=None, max_workgroups: int = 0, wide: bool = False) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``expected_q_values`` of agents/dqn.py:96-99 in one forward-only kernel -> (y, next_q - both float32 [B] -, next_action uint8 [B]).
    ``next_state`` float32 [M, F] (any row stride >= F) and ``reward`` float32 [M] are the replay buffer, read in place through
    ``index`` (int64 [B] on the device; None: every row in order, B = M).  ``policy_net`` None: DQN, next_q = max_a Q_target(s', a) and
    next_action the target net's own argmax; a network: DDQN, next_action = argmax_a Q_policy(s', a) (a second launch) and
    next_q = Q_target(s', next_action) - the per-row target, not the [B, B, 1] broadcast of agents/dqn.py:132-135 (module docstring).
    y = reward + gamma * next_q.  Nothing here is differentiated.  ``wide=True``: up to 128 input features."""
    what = "td_target"
    for net in (target_net,) + ((policy_net,) if policy_net is not None else ()):
        why = refusal(net, 2, wide=wide)
        if why:
            raise ValueError("%s: %s" % (what, why))
    fc = L.fc_layers(target_net)
    dev, M, ld, B = L.check_rows(fc, next_state, index, what)
    L.whole(reward, torch.float32, M, dev, what, "reward")
    pdesc = L.mlp_desc(L.fc_layers(policy_net)) if policy_net is not None else None
    y = torch.empty(B, dtype=torch.float32, device=dev)
    next_q = torch.empty(B, dtype=torch.float32, device=dev)
    next_action = torch.empty(B, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _target_launch(L.mlp_desc(fc), pdesc, next_state, ld, reward, index, B, y, next_q, next_action, L.stream(dev), gamma, max_workgroups, wide)
    return y, next_q, next_action


def q_loss_backward(policy_net, state: torch.Tensor, action: torch.Tensor, y: torch.Tensor, index: Optional[torch.Tensor] = None,
                    grad_clamp: float = 1.0, want_q: bool = False, max_workgroups: int = 0, wide: bool = False):
    """``nn.SmoothL1Loss()(Q(s, a), y)``, ``backward()`` and ``param.grad.data.clamp_(-grad_clamp, grad_clamp)`` of agents/dqn.py:93,
    102-109 in one kernel and its reduction: fills ``p.grad`` of the six parameters of ``policy_net`` (allocated where None, overwritten
    otherwise) and returns the loss (0-dim device tensor) [and Q(s, a), float32 [B]].  ``state`` float32 [M, F] and ``action`` int64 [M]
    are the replay buffer, read in place through ``index``; ``y`` float32 [B] (``td_target``'s) in minibatch order.
    ``grad_clamp=float("inf")``: no clamp.  ``wide=True``: up to 128 input features."""
    what = "q_loss_backward"
    why = refusal(policy_net, 2, wide=wide)
    if why:
        raise ValueError("%s: %s" % (what, why))
    fc = L.fc_layers(policy_net)
    dev, M, ld, B = L.check_rows(fc, state, index, what)
    L.whole(action, torch.int64, M, dev, what, "action")
    L.whole(y, torch.float32, B, dev, what, "y")
    if not float(grad_clamp) > 0.0:
        raise ValueError("%s: grad_clamp must be positive (inf: no clamp)" % what)
    desc = L.mlp_desc(fc)
    floats, nbytes = L.mlp_sizes(desc, B, max_workgroups, wide)
    flat = L.flat_grad(policy_net, floats, dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    q = torch.empty(B, dtype=torch.float32, device=dev) if want_q else None
    with torch.cuda.device(dev):
        _grad_launch(desc, state, ld, action, y, index, B, L.workspace(dev, nbytes), flat, loss, q, L.stream(dev), grad_clamp, max_workgroups, wide)
    L.publish(L.mlp_params(fc), flat, L.KEEP)
    return (loss, q) if want_q else loss


class DeviceReplayBuffer(L.RingBuffer):
    """``ReplayBuffer`` (agents/buffer.py:12-31: a ``deque(maxlen=capacity)`` of Transition tuples) as four preallocated tensors on
    ``device`` - ``state`` [capacity, F], ``next_state`` [capacity, F], ``action`` int64 [capacity], ``reward`` [capacity] - written as
    a ring (``_learner.RingBuffer``).  ``push``: ``n`` transitions at once, ``state`` / ``next_state`` [n, F], ``action`` / ``reward``
    [n] or [n, 1]; ``push_batch``: the dict of ``collect_dqn_transitions``, stored in (t, agent) order."""

    def __init__(self, capacity: int, num_state: int, device):
        if int(capacity) <= 0 or int(num_state) <= 0:
            raise ValueError("DeviceReplayBuffer: capacity and num_state must be positive")
        super().__init__(capacity, (), num_state, device)

    def _rows(self, n, state, next_state, action, reward):
        if state.shape != (n, self.num_state) or next_state.shape != (n, self.num_state) or action.numel() != n or reward.numel() != n:
            raise ValueError("DeviceReplayBuffer.push: state / next_state [n, %d], action and reward of n elements" % self.num_state)
        return state, next_state, action.reshape(n), reward.reshape(n)

    def sample(self, batch_size: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``batch_size`` positions (int64 on the device) drawn uniformly WITH replacement from the filled part, as ``random.choices``
        draws them (agents/buffer.py:26-27)."""
        if self._len == 0:
            raise ValueError("DeviceReplayBuffer.sample: the buffer is empty")
        return torch.randint(0, self._len, (int(batch_size),), generator=generator, device=self.device, dtype=torch.int64)


class DQNLearner:
    """``DQN`` / ``DDQN`` of agents/dqn.py without the acting half: the policy net, a target net of the same shape loaded from it
    (:33-35), the replay buffer and the optimiser; ``store`` and ``update``.

    ``double=False``: ``DQN.update``; ``True``: ``DDQN.update`` with the per-row target (module docstring).  ``soft_update=False`` leaves
    the target net alone after an update, as the reference's DDQN does.  ``backend="hip"``: target, loss and clamped gradient from
    the kernels (ValueError for networks they refuse); ``"torch"``: the reference's expressions under autograd with
    ``p.grad.clamp_(-1, 1)`` - the comparator and the fallback; ``"auto"``: the kernels where ``supported()`` holds and the minibatch
    has at least ``AUTO_MIN_ROWS`` rows, torch otherwise.  The optimiser step and the target blend are torch on every backend unless
    ``optimizer=mdr_amd.optim.FusedAdam``: then, with ``soft_update``, both are one ``FusedAdam.step(target=..., tau=...)``.
    ``wide=True``: the wide entry points, so a Q-network of up to 128 input features (both message flags on: 121) takes the kernels,
    eager or ``graph=True``; ``"auto"`` then takes them from ``AUTO_MIN_ROWS_WIDE`` minibatch rows on."""

    GRAD_CLAMP = 1.0      # agents/dqn.py:108-109

    def __init__(self, policy_net, lr: float, gamma: float = 0.99, tau: float = 0.01, buffer_capacity: int = 524288, batch_size: int = 256,
                 double: bool = False, backend: str = "auto", optimizer=torch.optim.Adam, soft_update: bool = True,
                 sampler: Optional[str] = None, graph: bool = False, wide: bool = False):
        L.check_backend(backend)
        self.wide = bool(wide)
        if backend == "hip":
            L.require(refusal(policy_net, 2, wide=self.wide), "DQNLearner")
        fc = getattr(policy_net, "fc", None)
        if fc is None or not all(isinstance(m, nn.Linear) for m in fc):
            raise ValueError("DQNLearner: policy_net needs the reference's `fc` ModuleList of Linear layers")
        self.policy_net = policy_net
        dev = fc[0].weight.device
        self.target_net = QNetworkMLP(fc[0].in_features, fc[-1].out_features, [m.out_features for m in list(fc)[:-1]]).to(dev)
        self.target_net.load_state_dict({k: v for k, v in policy_net.state_dict().items() if k.startswith("fc.")})
        self.gamma, self.tau = float(gamma), float(tau)
        self.batch_size, self.double, self.soft_update = int(batch_size), bool(double), bool(soft_update)
        self.backend = backend
        self.buffer = DeviceReplayBuffer(buffer_capacity, fc[0].in_features, dev)
        self.optimizer = optimizer(policy_net.parameters(), lr)
        # FusedAdam blends in its own launch where the optimiser's parameters are exactly the six the target net mirrors
        mine = L.mlp_params(fc)
        held = list(policy_net.parameters())
        same = len(held) == len(mine) and all(a is b for a, b in zip(held, mine))
        self._fused_target = L.mlp_params(self.target_net.fc) if same else None
        self.training_step = 0
        self.before_step = None      # optional callable(learner): runs after the backward (and the clamp) of an update, before the optimiser
        # sampler="philox": the positions from csrc/mdr_minibatch.hip by (seed, training_step) instead of a torch.Generator;
        # graph=True: every update replayed from one captured graph (graph_update.py)
        self.sampler, self.graph = L.check_sampler(sampler, graph), bool(graph)
        self.graph_captures = 0
        self._graph = None
        if self.graph:
            why = graph_update.refusal(backend, self.sampler, (self.optimizer,), self.uses_kernels(max(self.batch_size, 1)))
            if not why and self.soft_update and self._fused_target is None:
                why = "the optimiser's parameters are not the six tensors the target net mirrors (the blend would be torch launches)"
            if why:
                raise ValueError("DQNLearner(graph=True): " + why)

    @classmethod
    def from_config(cls, dqn_prop: dict, policy_net, double: bool = False, backend: str = "auto", optimizer=torch.optim.Adam,
                    soft_update: bool = True, sampler: Optional[str] = None, graph: bool = False, wide: bool = False) -> "DQNLearner":
        """From the reference's ``config_dict["DQN_prop"]`` (agents/dqn.py:23-29)."""
        return cls(policy_net, dqn_prop["lr"], gamma=dqn_prop["gamma"], tau=dqn_prop["tau"], buffer_capacity=dqn_prop["buffer_capacity"],
                   batch_size=dqn_prop["batch_size"], double=double, backend=backend, optimizer=optimizer, soft_update=soft_update,
                   sampler=sampler, graph=graph, wide=wide)

    def uses_kernels(self, nb_rows: int) -> bool:
        if self.backend == "auto":
            return (refusal(self.policy_net, 2, wide=self.wide) is None and refusal(self.target_net, 2, wide=self.wide) is None
                    and nb_rows >= (AUTO_MIN_ROWS_WIDE if self.wide else AUTO_MIN_ROWS))
        return self.backend == "hip"

    def _kernels(self):
        """(sizes, target launch, gradient launch) of the calls ``loss_backward`` makes, this learner's fixed arguments bound: what a
        captured graph runs on its static buffers (graph_update.DQNUpdateGraph)."""
        return (partial(L.mlp_sizes, wide=self.wide), partial(_target_launch, gamma=self.gamma, wide=self.wide),
                partial(_grad_launch, grad_clamp=self.GRAD_CLAMP, wide=self.wide))

    def store(self, batch: Dict[str, torch.Tensor]) -> None:
        """``store_transition`` (agents/dqn.py:58-63) for every transition of a ``collect_dqn_transitions`` dict."""
        self.buffer.push_batch(batch)

    def sample(self, seed: int) -> torch.Tensor:
        """The minibatch of this update: ``buffer.sample`` under a ``torch.Generator`` seeded by (seed, training_step) - the same
        positions whatever the backend."""
        if self.sampler == "philox":      # one Philox word per position by (seed, training_step), one launch (graph_update.sample)
            if len(self.buffer) == 0:
                raise ValueError("DeviceReplayBuffer.sample: the buffer is empty")
            return graph_update.sample(self.batch_size, len(self.buffer), seed, self.training_step, self.buffer.device)
        return self.buffer.sample(self.batch_size, L.seeded_generator(seed, self.training_step, self.buffer.device))

    def _capture(self):
        """Capture the graph of one update without replaying it; both nets, the moments and every counter are what they were."""
        self._graph = graph_update.DQNUpdateGraph(self)
        self.graph_captures += 1
        return self._graph

    def update_target_network(self) -> None:
        """agents/dqn.py:77-82: params = (1 - tau) * params + tau * new over the six tensors (two fused launches)."""
        L.blend(L.mlp_params(self.target_net.fc), L.mlp_params(self.policy_net.fc), self.tau)

    def loss_backward(self, index: torch.Tensor) -> torch.Tensor:
        """Target, Huber loss, backward and the clamp for the transitions at ``index``: fills the policy net's ``.grad``."""
        buf = self.buffer
        if self.uses_kernels(int(index.shape[0])):
            y, _, _ = td_target(self.target_net, buf.next_state, buf.reward, self.gamma, index=index,
                                policy_net=self.policy_net if self.double else None, wide=self.wide)
            return q_loss_backward(self.policy_net, buf.state, buf.action, y, index=index, grad_clamp=self.GRAD_CLAMP, wide=self.wide)
        state, action, reward, next_state = buf.state[index], buf.action[index].view(-1, 1), buf.reward[index].view(-1, 1), buf.next_state[index]
        q_values = self.policy_net(state).gather(1, action)
        with torch.no_grad():
            if self.double:
                next_action = self.policy_net(next_state).argmax(dim=1, keepdim=True)
                next_q_values = self.target_net(next_state).gather(1, next_action)      # [B, 1]: the per-row target
            else:
                next_q_values = self.target_net(next_state).max(1)[0].unsqueeze(1)
        expected_q_values = reward + (next_q_values * self.gamma)
        loss = nn.SmoothL1Loss()(q_values, expected_q_values)
        self.optimizer.zero_grad()
        loss.backward()
        for param in self.policy_net.parameters():
            param.grad.clamp_(-self.GRAD_CLAMP, self.GRAD_CLAMP)
        return loss.detach()

    def update(self, seed: int = 0) -> Optional[torch.Tensor]:
        """One ``update()`` of agents/dqn.py:84-112: sample -> TD target -> loss, backward and clamp -> ``optimizer.step()`` ->
        ``update_target_network()``.  -> the loss (0-dim device tensor), or None while the buffer holds fewer than ``batch_size``
        transitions (:85-86).  ``graph=True``: the same launches replayed from a captured graph, the same bits as the eager
        ``sampler="philox"`` update."""
        if self.graph:
            return graph_update.dqn_update(self, seed)
        if len(self.buffer) < self.batch_size:
            return None
        loss = self.loss_backward(self.sample(seed))
        if self.before_step is not None:
            self.before_step(self)
        if self.soft_update and isinstance(self.optimizer, FusedAdam) and self._fused_target is not None:
            self.optimizer.step(target=self._fused_target, tau=self.tau)      # Adam and the blend in one launch
        else:
            self.optimizer.step()
            if self.soft_update:
                self.update_target_network()
        self.training_step += 1
        return loss


def train_dqn(env, learner: DQNLearner, nb_steps: int, updates_per_step: int = 1, epsilon: float = 1.0, epsilon_decay: float = 0.99998,
              min_epsilon: float = 0.01, seed: int = 0) -> Tuple[torch.Tensor, float]:
    """The loop of train_dqn.py:54-91 on a batched env (reset by the caller): every iteration one ``collect_dqn_transitions`` step of
    all envs under the learner's policy net, ``store``, then ``updates_per_step`` updates.  -> (the losses of the updates that ran,
    float32 [n] on the device, and the final epsilon; the defaults are ``DQN_prop``'s ``epsilon_decay`` and ``min_epsilon``).
    The reference stores its N agents' transitions and then updates ONCE per env step (train_dqn.py:81-89): ``updates_per_step=1``
    with one env matches its update count.  E envs store E N transitions per iteration; ``updates_per_step`` is the batched stand-in
    for the updates the reference would have made on that many transitions (``updates_per_step=E`` keeps its updates per transition)."""
    from .rollout import collect_dqn_transitions
    losses = []
    eps = float(epsilon)
    for t in range(int(nb_steps)):
        batch = collect_dqn_transitions(env, learner.policy_net, 1, epsilon=eps, epsilon_decay=epsilon_decay, min_epsilon=min_epsilon,
                                        seed=(int(seed) * 1000003 + t) & (2 ** 63 - 1))
        eps = batch["epsilon"]
        learner.store(batch)
        for _ in range(int(updates_per_step)):
            loss = learner.update(seed=seed)
            if loss is not None:
                losses.append(loss)
    dev = learner.buffer.device
    return (torch.stack(losses) if losses else torch.empty(0, dtype=torch.float32, device=dev)), eps
