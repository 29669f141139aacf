"""Run the reference's own ``update()`` of a learner and record it  --  TEST INFRASTRUCTURE ONLY (tests/golden/make_learner_golden.py).

The reference is imported through oracle/ref_harness.py from where it lies; nothing of it is copied and nothing is written into its
tree.  Per case: build the reference learner from ``config_dict`` with a small override, fill its buffer with synthetic transitions in
the order the reference's training script stores them, and run ``update()`` twice from the same initial weights:

  ref32   the reference as shipped, float32
  ref64   the same reference code with the nets ``.double()`` and fresh Adam optimisers over them.  The reference hard-codes
          ``dtype=torch.float``; for the run the name ``torch`` in that one reference module is bound to a proxy that forwards
          everything to torch except ``float`` (``torch.float64``) and is restored afterwards.

Nothing random stays implicit: ref32 records the minibatch index lists (``BatchSampler(SubsetRandomSampler(..))`` of PPO / MAPPO,
``random.choices`` of ``ReplayBuffer.sample``, ``np.random.choice`` of ``MADDPG.sample``) and what every ``Tensor.exponential_`` of
``F.gumbel_softmax`` returned, and ref64 replays them.  Recorded are the initial state_dicts, ``Gt``, at the first
minibatch both losses and the gradients of every net as ``clip_grad_norm_`` meets them (DQN, which has no clip: the clamped gradients
at the optimiser's step pre-hook), after every minibatch the losses and those gradients' norm, and the parameters of every net after
the first step and after the last.

Storage (the fixtures must stay small; the nets are the reference's 100-100): float64 arrays are stored as the nearest float32
(``<key>``) plus the remainder in 2^-15 of that float32's spacing as int16 (``<key>@lo``): 6 bytes, relative error below 2^-39.
Parameter checkpoints keep, of a tensor of more than CKPT_MAX elements, every ``step``-th element of the flattened tensor with
``step`` coprime to the row length, so that every row and every column is met (``ckpt_positions``); the first-minibatch gradients
are whole.

The wrappers (``Tensor.backward``, ``Tensor.exponential_``, ``clip_grad_norm_`` and, for the MADDPG twin, ``Tensor.float``) are set
on the classes for the length of one reference run and put back in ``finally``: while a run lasts they hold for the whole process,
so ``generate`` - and the live re-run test that calls it - must not run next to other torch work in parallel threads.

The weights and states lie on the dyadic grids of tests/ppo_grad_ref.py / tests/dqn_grad_ref.py, the precondition of those modules'
derived bounds (exact pre-activations, so no ReLU mask and no argmax is a matter of rounding at the first minibatch).  TarMAC-PPO's
critic and states lie on tests/tarmac_critic_ref.py's grids; its actor is the reference's own init, scaled as
tests/golden/make_tarmac_golden.py scales it, under tests/tarmac_ppo_ref.py's ReLU condition.  ``TarMAC_PPO.update`` builds ``Gt``
with ``torch.cat``: the proxy remembers that call's latest result too.
"""
from __future__ import annotations

import contextlib
import copy
import io
import math
import os
import sys
import zipfile
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_harness  # noqa: E402

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
CKPT_MAX = 256
CASES = ("ppo_f51", "ppo_f21_zero", "mappo", "dqn", "dqn_clamped", "ddqn_b1", "maddpg_agents", "maddpg_shared", "tarmac_ppo")
FC_KEYS = ("fc.0.weight", "fc.0.bias", "fc.1.weight", "fc.1.bias", "fc.2.weight", "fc.2.bias")
NET_KEYS = ("net.0.weight", "net.0.bias", "net.2.weight", "net.2.bias", "net.4.weight", "net.4.bias")      # DDPG_Network
GRID_KEYS = ("W1", "b1", "W2", "b2", "W3", "b3")


def path(case: str) -> str:
    return os.path.join(GOLDEN_DIR, "learner_%s.npz" % case)


# -- storage --------------------------------------------------------------------------------------------------------------------------
def split64(a):
    """float64 -> (float32 hi, int16 lo): a ~ hi + lo * spacing(hi) / 2^15."""
    a = np.asarray(a, dtype=np.float64)
    hi = a.astype(np.float32)
    sp = np.spacing(np.abs(hi)).astype(np.float64)
    lo = np.rint((a - hi.astype(np.float64)) / sp * 32768.0)
    return hi, np.clip(lo, -32767, 32767).astype(np.int16)


def join64(hi, lo):
    hi = np.asarray(hi, dtype=np.float32)
    return hi.astype(np.float64) + lo.astype(np.float64) * np.spacing(np.abs(hi)).astype(np.float64) / 32768.0


def put64(out, key, a):
    out[key], out[key + "@lo"] = split64(a)


def ckpt_positions(shape) -> np.ndarray:
    """The flat positions a checkpoint keeps of a tensor of ``shape``."""
    n = int(np.prod(shape))
    if n <= CKPT_MAX:
        return np.arange(n)
    cols = int(shape[-1])
    step = -(-n // CKPT_MAX)
    while math.gcd(step, cols) != 1:
        step += 1
    return np.arange(0, n, step)


def write_npz(file: str, arrays: dict) -> None:
    """A compressed .npz with fixed member dates and order: the same arrays give the same bytes."""
    with zipfile.ZipFile(file, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.array(arrays[key], order="C"), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


# -- instrumentation ------------------------------------------------------------------------------------------------------------------
class _Run:
    """What one run of the reference drew and produced; ``replay``: the run whose draws this one replays."""

    def __init__(self, replay=None):
        self.replay = replay
        self.draws = []           # index lists, in call order
        self.losses = []          # float(loss) of every backward(), in call order
        self.norms = {}           # net -> [gradient norm at every clip / step pre-hook]
        self.first_grads = {}     # net -> flat float64 gradient at the first of them
        self.ckpt = {}            # "first" / "last" -> {net: {key: float64 array}}
        self.noise = []           # what every Tensor.exponential_ returned, in call order
        self.Gt = None
        self.last_tensor = None
        self.last_cat = None      # TarMAC_PPO.update builds Gt with torch.cat and drops its last row (agents/tarmac_ppo.py:135-141)

    def snapshot(self, tag, nets):
        self.ckpt[tag] = {n: {k: v.detach().double().numpy().copy() for k, v in net.state_dict().items()} for n, net in nets.items()}

    def meet_grads(self, name, params):
        flat = np.concatenate([p.grad.detach().double().numpy().reshape(-1) for p in params if p.grad is not None])
        self.first_grads.setdefault(name, flat.copy())
        return flat


class _TorchProxy:
    """``torch`` for one reference module: everything is torch's, except ``float`` (the run's dtype) and ``tensor``, whose latest
    result is remembered (the last tensor the update builds before its minibatch loop is ``Gt``)."""

    def __init__(self, run, float_dtype):
        self._run, self._float = run, float_dtype

    def __getattr__(self, name):
        import torch
        if name == "float":
            return self._float
        if name == "cat":
            def cat(*args, **kw):
                out = torch.cat(*args, **kw)
                self._run.last_cat = out
                return out
            return cat
        if name == "tensor":
            def tensor(*args, **kw):
                out = torch.tensor(*args, **kw)
                self._run.last_tensor = out
                return out
            return tensor
        return getattr(torch, name)


class _NumpyProxy:
    """``np`` for agents/ddpg.py: ``np.random.choice`` (MADDPG.sample) records its draw or replays the recorded one."""

    def __init__(self, run):
        self._run = run
        self.random = self

    def choice(self, a, size=None, replace=True, p=None):
        run = self._run
        idx = run.replay.draws[len(run.draws)] if run.replay is not None else np.random.choice(a, size=size, replace=replace, p=p)
        run.draws.append([int(i) for i in idx])
        return np.array(run.draws[-1], dtype=np.int64)

    def __getattr__(self, name):
        return getattr(np, name)


class _RandomProxy:
    """``random`` for agents/buffer.py: ``choices`` draws positions with the true ``random.choices`` (the same draws as on the
    population itself), records them, or replays the recorded ones."""

    def __init__(self, run):
        self._run = run

    def choices(self, population, k=1):
        import random
        run = self._run
        idx = run.replay.draws[len(run.draws)] if run.replay is not None else random.choices(range(len(population)), k=k)
        run.draws.append([int(i) for i in idx])
        return [population[i] for i in idx]

    def __getattr__(self, name):
        import random
        return getattr(random, name)


@contextlib.contextmanager
def _instrumented(run, module, nets, double, buffer_module=None, maddpg=False):
    """The reference ``module`` under the proxies and wrappers above, everything restored on exit.  ``nets``: name -> module."""
    import torch
    owner = {id(p): n for n, net in nets.items() for p in net.parameters()}
    saved_torch, saved_sampler = module.torch, getattr(module, "BatchSampler", None)
    real_clip, real_backward = torch.nn.utils.clip_grad_norm_, torch.Tensor.backward
    saved_random = buffer_module.random if buffer_module is not None else None

    def batch_sampler(sampler, batch_size, drop_last):
        if run.Gt is None:
            run.Gt = (run.last_cat[:-1] if run.last_cat is not None else run.last_tensor).detach().clone()
        epoch = len(run.draws)
        lists = run.replay.draws[epoch] if run.replay is not None else [[int(i) for i in b] for b in saved_sampler(sampler, batch_size, drop_last)]
        run.draws.append(lists)
        return lists

    def clip(parameters, max_norm, *args, **kw):
        params = list(parameters)
        name = owner[id(params[0])]
        run.meet_grads(name, params)
        norm = real_clip(params, max_norm, *args, **kw)
        run.norms.setdefault(name, []).append(float(norm))
        return norm

    def backward(self, *args, **kw):
        run.losses.append(float(self.detach()))
        return real_backward(self, *args, **kw)

    real_exponential, real_float, saved_np = torch.Tensor.exponential_, torch.Tensor.float, getattr(module, "np", None)

    def exponential_(self, *args, **kw):      # the noise of every F.gumbel_softmax, in call order
        if run.replay is not None:
            self.copy_(run.replay.noise[len(run.noise)].to(self.dtype))
        else:
            real_exponential(self, *args, **kw)
        run.noise.append(self.detach().clone())
        return self

    if maddpg:
        torch.Tensor.exponential_ = exponential_
        module.np = _NumpyProxy(run)
        if double:      # DDPGBuffer.sample calls .float() on what it read (agents/buffer.py:75-89): the twin keeps float64
            torch.Tensor.float = lambda self, *args, **kw: self.double()
    module.torch = _TorchProxy(run, torch.float64 if double else torch.float32)
    if saved_sampler is not None:
        module.BatchSampler = batch_sampler
    if buffer_module is not None:
        buffer_module.random = _RandomProxy(run)
    torch.nn.utils.clip_grad_norm_ = clip
    torch.Tensor.backward = backward
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            yield
    finally:
        module.torch = saved_torch
        if saved_sampler is not None:
            module.BatchSampler = saved_sampler
        if buffer_module is not None:
            buffer_module.random = saved_random
        torch.nn.utils.clip_grad_norm_ = real_clip
        torch.Tensor.backward = real_backward
        torch.Tensor.exponential_, torch.Tensor.float = real_exponential, real_float
        if maddpg:
            module.np = saved_np


def _quiet(fn, *args, **kw):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kw)


def _load(net, sd, double):
    import torch
    net.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in sd.items()})
    return net.double() if double else net


def _fc_state(grid):
    return {k: np.array(grid[g], dtype=np.float32) for k, g in zip(FC_KEYS, GRID_KEYS)}


def _config(section, **override):
    cfg = copy.deepcopy(ref_harness.load_reference()["config_dict"])
    cfg[section].update(override)
    return cfg


def _pack(out, runs, nets_init, loss_names):
    """The recorded results of (ref32, ref64) into ``out``."""
    losses_per_step = len(loss_names)
    out["meta/loss_names"] = np.array(loss_names)
    for name, sd in nets_init.items():
        for k, v in sd.items():
            out["init/%s/%s" % (name, k)] = np.asarray(v, dtype=np.float32)
    for tag, run in zip(("ref32", "ref64"), runs):
        put64(out, tag + "/loss", np.array(run.losses, dtype=np.float64).reshape(-1, losses_per_step))
        for name, series in run.norms.items():
            put64(out, "%s/norm/%s" % (tag, name), np.array(series, dtype=np.float64))
        if run.Gt is not None:
            put64(out, tag + "/Gt", run.Gt.double().numpy())
        for ck, nets in run.ckpt.items():
            for name, sd in nets.items():
                for k, v in sd.items():
                    kept = v.reshape(-1)[ckpt_positions(v.shape)]
                    if tag == "ref32":
                        out["ref32/%s/%s/%s" % (ck, name, k)] = kept.astype(np.float32)      # exact: the run is float32
                    else:
                        put64(out, "ref64/%s/%s/%s" % (ck, name, k), kept)
    for name, g in runs[1].first_grads.items():
        put64(out, "ref64/grad/%s" % name, g)


# -- PPO and MAPPO --------------------------------------------------------------------------------------------------------------------
PPOTransition = namedtuple("Transition", ["state", "action", "a_log_prob", "reward", "next_state", "done"])
MAPPOTransition = namedtuple("Transition", ["state", "action", "others_actions", "a_log_prob", "reward", "next_state", "done"])


def _ppo_data(F, layers, critic_in, T, A, seed):
    """Grid states [T + 1, A, F], grid weights of both nets, actions, rewards and old probabilities = the initial actor's own
    probability of the action x U(0.7, 1.4), kept in (0.02, 0.98] and at least 1e-3 away from a ratio on a clip bound."""
    from tests import ppo_grad_ref as pr
    rows = (T + 1) * A
    da = pr.draw(F, layers[0], layers[1], 2, rows=rows, seed=seed)
    dc = pr.draw(critic_in, layers[0], layers[1], 1, rows=rows, seed=seed)
    r = np.random.default_rng([seed, 0xA11, F, T, A])
    state = np.array(da["x"]).reshape(T + 1, A, F)
    action = r.integers(0, 2, (T, A)).astype(np.int64)
    reward = r.standard_normal((T, A)).astype(np.float32)
    logits = pr.forward(dict(da, x=state[:T].reshape(-1, F)), np.float64)["l"]
    a = action.reshape(-1)
    dd = logits[np.arange(T * A), a] - logits[np.arange(T * A), 1 - a]
    p = 1.0 / (1.0 + np.exp(-dd))
    old = np.clip(p * r.uniform(0.7, 1.4, T * A), 0.02 + 1e-6, 0.98).astype(np.float32)
    for _ in range(8):
        ratio = p / old.astype(np.float64)
        close = (np.abs(ratio - (1 - pr.CLIP)) < 1e-3) | (np.abs(ratio - (1 + pr.CLIP)) < 1e-3)
        if not close.any():
            break
        old = np.where(close, np.minimum(old * np.float32(0.99), np.float32(0.98)), old).astype(np.float32)
    return dict(state=state, action=action, reward=reward, a_prob=old.reshape(T, A), actor=_fc_state(da), critic=_fc_state(dc))


def _run_ppo_like(kind, cfg, F, nb_agents, data, done, order, double, replay, seed):
    """One run of agents/ppo.py's or agents/mappo.py's ``update``.  ``order``: 'agent' (each agent's steps in turn) or 'step' (step by
    step, the agents interleaved: train_mappo.py:86); PPO's own buffer is per agent whatever the order of the calls."""
    import torch
    ref_harness.load_reference()
    opt = SimpleNamespace(net_seed=seed, no_wandb=True, nb_agents=nb_agents)
    if kind == "ppo":
        import agents.ppo as module
        learner = _quiet(module.PPO, cfg, opt, num_state=F)
    else:
        import agents.mappo as module
        learner = _quiet(module.MAPPO, cfg, opt, num_state=F)
    learner.actor_net = _load(learner.actor_net, data["actor"], double)
    learner.critic_net = _load(learner.critic_net, data["critic"], double)
    learner.actor_optimizer = torch.optim.Adam(learner.actor_net.parameters(), learner.lr_actor)
    learner.critic_net_optimizer = torch.optim.Adam(learner.critic_net.parameters(), learner.lr_critic)
    T, A = data["action"].shape
    pairs = [(t, a) for t in range(T) for a in range(A)] if order == "step" else [(t, a) for a in range(A) for t in range(T)]
    for t, a in pairs:
        common = dict(state=data["state"][t, a], action=int(data["action"][t, a]), a_log_prob=float(data["a_prob"][t, a]),
                      reward=float(data["reward"][t, a]), next_state=data["state"][t + 1, a], done=bool(done[t, a]))
        if kind == "ppo":
            learner.store_transition(PPOTransition(**common), a)
        else:
            env0 = (a // nb_agents) * nb_agents
            others = [int(data["action"][t, k]) for k in range(env0, env0 + nb_agents) if k != a]
            learner.store_transition(MAPPOTransition(others_actions=others, **common))
    run = _Run(replay)
    nets = {"actor": learner.actor_net, "critic": learner.critic_net}
    steps = [0]

    def after_critic_step(optimizer, args, kwargs):      # the critic's step ends a minibatch (agents/ppo.py:187)
        steps[0] += 1
        if steps[0] == 1:
            run.snapshot("first", nets)

    learner.critic_net_optimizer.register_step_post_hook(after_critic_step)
    run.bootstrap = np.zeros((T, A), dtype=np.float64)
    if kind == "ppo" and not learner.zero_eoepisode_return:      # agents/ppo.py:131, before the update moves the critic
        dtype = torch.float64 if double else torch.float32
        for t, a in pairs:
            if done[t, a]:
                run.bootstrap[t, a] = learner.get_value(torch.tensor(data["state"][t + 1, a], dtype=dtype))
    torch.manual_seed(seed + 77)      # SubsetRandomSampler draws from torch's global generator
    with _instrumented(run, module, nets, double):
        learner.update(0)
    if run.Gt is None:
        run.Gt = run.last_tensor.detach().clone()
    run.snapshot("last", nets)
    run.training_step = int(learner.training_step)
    return run


def make_ppo(case, F, zero, seed):
    T, A, layers = 12, 10, [100, 100]
    cfg = _config("PPO_prop", actor_layers=layers, critic_layers=layers, batch_size=50, ppo_update_time=2, zero_eoepisode_return=zero)
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = A
    data = _ppo_data(F, layers, F, T, A, seed)
    done = np.zeros((T, A), dtype=bool)
    done[T - 1] = True
    r32 = _run_ppo_like("ppo", cfg, F, A, data, done, "step", False, None, seed)
    r64 = _run_ppo_like("ppo", cfg, F, A, data, done, "step", True, r32, seed)
    return _ppo_out(cfg["PPO_prop"], "ppo", F, A, T, A, zero, data, done, (r32, r64))      # Gt in the reference's order a T + t


def _ppo_out(prop, kind, F, nb_agents, T, A, zero, data, done, runs):
    out = {"meta/kind": np.array(kind), "meta/F": np.int64(F), "meta/nb_agents": np.int64(nb_agents), "meta/T": np.int64(T), "meta/A": np.int64(A),
           "meta/zero_eoepisode_return": np.int64(zero), "meta/training_step": np.int64(runs[0].training_step)}
    for k in ("gamma", "lr_actor", "lr_critic", "clip_param", "max_grad_norm"):
        out["meta/" + k] = np.float64(prop[k])
    for k in ("batch_size", "ppo_update_time"):
        out["meta/" + k] = np.int64(prop[k])
    out.update({"in/state": data["state"], "in/action": data["action"], "in/reward": data["reward"], "in/a_prob": data["a_prob"],
                "in/done": done})
    flat = [b for epoch in runs[0].draws for b in epoch]
    index = np.full((len(flat), max(len(b) for b in flat)), -1, dtype=np.int64)
    for i, b in enumerate(flat):
        index[i, :len(b)] = b
    out["draws/index"] = index
    out["draws/per_epoch"] = np.array([len(e) for e in runs[0].draws], dtype=np.int64)
    out["ref32/bootstrap"] = runs[0].bootstrap.astype(np.float32)      # exact: the run is float32
    _pack(out, runs, {"actor": data["actor"], "critic": data["critic"]}, ("actor", "critic"))
    return out


def make_mappo(case, seed):
    F, N, T, layers = 21, 4, 10, [36, 20]
    cfg = _config("MAPPO_prop", actor_layers=layers, critic_layers=layers, batch_size=16, ppo_update_time=2)
    data = _ppo_data(F, layers, F + N - 1, T, N, seed)
    done = np.zeros((T, N), dtype=bool)
    done[4] = done[T - 1] = True      # train_mappo.py:76: one flag for the whole step
    r32 = _run_ppo_like("mappo", cfg, F, N, data, done, "step", False, None, seed)
    r64 = _run_ppo_like("mappo", cfg, F, N, data, done, "step", True, r32, seed)
    out = _ppo_out(cfg["MAPPO_prop"], "mappo", F, N, T, N, 1, data, done, (r32, r64))
    # the same transitions stored agent by agent: only Gt is wanted of this run (no epochs)
    cfg0 = _config("MAPPO_prop", actor_layers=layers, critic_layers=layers, batch_size=16, ppo_update_time=0)
    by_agent = _run_ppo_like("mappo", cfg0, F, N, data, done, "agent", False, None, seed)
    put64(out, "ref32/Gt_by_agent", by_agent.Gt.double().numpy())      # [N, T] flattened
    return out


# -- DQN and DDQN ---------------------------------------------------------------------------------------------------------------------
def _dqn_data(F, layers, rows, seed, reward_scale, w3_scale):
    from tests import dqn_grad_ref as dq
    d = dq.draw(F, layers[0], layers[1], rows=rows, seed=seed)
    d = {k: np.array(v) for k, v in d.items()}
    d["W3"] = (d["W3"] * np.float32(w3_scale)).astype(np.float32)      # a power of two: still dyadic (z1, z2 do not depend on it)
    for g in GRID_KEYS:      # the reference's target net starts as a copy of the policy net (agents/dqn.py:35)
        d["t" + g] = d[g].copy()
    d["reward"] = (d["reward"] * np.float32(reward_scale)).astype(np.float32)
    return d


def _run_dqn(double_q, cfg, F, d, nb_updates, double, replay, seed):
    import torch
    ref_harness.load_reference()
    import agents.buffer as buffer_module
    import agents.dqn as module
    opt = SimpleNamespace(net_seed=seed, save_actor_name=None)
    learner = _quiet((module.DDQN if double_q else module.DQN), cfg, opt, num_state=F)
    sd = _fc_state(d)
    learner.policy_net = _load(learner.policy_net, sd, double)
    learner.target_net = _load(learner.target_net, sd, double)
    learner.policy_optimizer = torch.optim.Adam(learner.policy_net.parameters(), learner.lr)
    run = _Run(replay)
    nets = {"policy": learner.policy_net, "target": learner.target_net}
    params = list(learner.policy_net.parameters())

    def before_step(optimizer, args, kwargs):      # the clamped gradient the optimiser takes (agents/dqn.py:108-110)
        flat = run.meet_grads("policy", params)
        run.norms.setdefault("policy", []).append(float(np.sqrt((flat * flat).sum())))

    learner.policy_optimizer.register_step_pre_hook(before_step)
    with _instrumented(run, module, nets, double, buffer_module):
        for i in range(d["x"].shape[0]):      # train_dqn.py:81: state, action, reward, next state
            learner.store_transition(d["x"][i], int(d["action"][i]), float(d["reward"][i]), d["xn"][i])
        for u in range(nb_updates):
            learner.update()
            if u == 0:
                run.snapshot("first", nets)
    run.snapshot("last", nets)
    run.training_step = nb_updates
    return run


def make_dqn(case, double_q, batch_size, reward_scale, seed, w3_scale=1.0):
    F, layers, rows, nb_updates = 21, [100, 100], 60, 5
    cfg = _config("DQN_prop", network_layers=layers, batch_size=batch_size, tau=0.01, buffer_capacity=4096)
    d = _dqn_data(F, layers, rows, seed, reward_scale, w3_scale)
    import random
    random.seed(seed + 99)      # ReplayBuffer.sample draws from the global ``random``
    r32 = _run_dqn(double_q, cfg, F, d, nb_updates, False, None, seed)
    r64 = _run_dqn(double_q, cfg, F, d, nb_updates, True, r32, seed)
    prop = cfg["DQN_prop"]
    out = {"meta/kind": np.array("ddqn" if double_q else "dqn"), "meta/F": np.int64(F), "meta/batch_size": np.int64(batch_size),
           "meta/training_step": np.int64(nb_updates), "meta/gamma": np.float64(prop["gamma"]), "meta/tau": np.float64(prop["tau"]),
           "meta/lr": np.float64(prop["lr"]),
           "in/state": d["x"], "in/next_state": d["xn"], "in/action": d["action"], "in/reward": d["reward"],
           "draws/index": np.array(r32.draws, dtype=np.int64)}
    _pack(out, (r32, r64), {"policy": _fc_state(d)}, ("policy",))
    return out


# -- MADDPG ---------------------------------------------------------------------------------------------------------------------------
def _maddpg_data(N, F, H, rows, shared, seed):
    """Env-steps and nets on ppo_grad_ref's grids (tests/maddpg_grad_ref.py's): one actor and one critic per agent (shared: one)."""
    from tests.ppo_grad_ref import _grid
    r = np.random.default_rng([seed, 0xDD6, N, F, H, rows])
    J = N * (F + 2)
    d = dict(state=_grid(r, -4, 4, 4, (rows, N, F)), next_state=_grid(r, -4, 4, 4, (rows, N, F)), reward=_grid(r, -12, 12, 4, (rows, N)))
    d = {k: v.astype(np.float32) for k, v in d.items()}
    d["action"] = r.integers(0, 2, (rows, N)).astype(np.int64)
    nets = {}
    for k in range(1 if shared else N):
        for kind, (K, O) in (("actor", (F, 2)), ("critic", (J, 1))):
            g = dict(W1=_grid(r, -4, 4, 8, (H, K)), b1=_grid(r, -8, 8, 32, H), W2=_grid(r, -4, 4, 64, (H, H)), b2=_grid(r, -8, 8, 32, H),
                     W3=_grid(r, -4, 4, 16, (O, H)), b3=_grid(r, -8, 8, 32, O))
            nets["%s%d" % (kind, k)] = {key: g[n].astype(np.float32) for key, n in zip(NET_KEYS, GRID_KEYS)}
    return d, nets


def _run_maddpg(cfg, N, F, d, init, shared, nb_updates, double, replay, seed):
    import logging
    import torch
    ref_harness.load_reference()
    import agents.ddpg as module
    opt = SimpleNamespace(net_seed=seed, no_wandb=True, nb_agents=N, DDPG_shared=int(shared))
    saved_logger = module.MADDPG.setup_logger
    module.MADDPG.setup_logger = lambda self, filename: logging.getLogger("learner_golden.null")      # never ./ddpg_results/maddpg.log
    try:
        learner = _quiet(module.MADDPG, cfg, opt, F, None)
    finally:
        module.MADDPG.setup_logger = saved_logger
    # ddpg.py:217-223 aliases the LAST agent's nets to agent 0's: with two agents that is full sharing
    own = [0] if shared else list(range(N))
    for k in own:
        ag = learner.agents[k]
        _load(ag.actor_net, init["actor%d" % k], double), _load(ag.critic_net, init["critic%d" % k], double)
        if double:
            ag.tgt_actor_net.double(), ag.tgt_critic_net.double()
        module.copy_model(ag.actor_net, ag.tgt_actor_net), module.copy_model(ag.critic_net, ag.tgt_critic_net)
        ag.actor_optimizer = torch.optim.Adam(ag.actor_net.parameters(), ag.lr_actor)
        ag.critic_optimizer = torch.optim.Adam(ag.critic_net.parameters(), ag.lr_critic)
    if shared:
        assert N == 2 and learner.agents[1].actor_net is learner.agents[0].actor_net and learner.agents[1].tgt_critic_net is learner.agents[0].tgt_critic_net
        learner.agents[1].actor_optimizer, learner.agents[1].critic_optimizer = learner.agents[0].actor_optimizer, learner.agents[0].critic_optimizer
    for i in range(d["state"].shape[0]):      # train_ddpg.py:111-115, every agent its own observation
        learner.push({k: d["state"][i, k] for k in range(N)}, {k: int(d["action"][i, k]) for k in range(N)},
                     {k: float(d["reward"][i, k]) for k in range(N)}, {k: d["next_state"][i, k] for k in range(N)}, {k: False for k in range(N)})
    nets = {}
    for k in own:
        ag = learner.agents[k]
        nets.update({"actor%d" % k: ag.actor_net, "critic%d" % k: ag.critic_net, "tgt_actor%d" % k: ag.tgt_actor_net, "tgt_critic%d" % k: ag.tgt_critic_net})
    run = _Run(replay)
    np.random.seed(seed + 5)
    torch.manual_seed(seed + 6)
    with _instrumented(run, module, nets, double, maddpg=True):
        for u in range(nb_updates):      # train_ddpg.py:124-131
            learner.update()
            learner.update_target()
            if u == 0:
                run.snapshot("first", nets)
    run.snapshot("last", nets)
    run.training_step = nb_updates
    return run


def make_maddpg(case, shared, seed):
    N, F, H, rows, B, nb_updates = (2 if shared else 3), 21, 32, 40, 24, 3
    cfg = _config("DDPG_prop", actor_hidden_dim=H, critic_hidden_dim=H, batch_size=B, buffer_capacity=64)
    d, init = _maddpg_data(N, F, H, rows, shared, seed)
    r32 = _run_maddpg(cfg, N, F, d, init, shared, nb_updates, False, None, seed)
    r64 = _run_maddpg(cfg, N, F, d, init, shared, nb_updates, True, r32, seed)
    prop = cfg["DDPG_prop"]
    import torch
    noise = torch.stack([-e.log() for e in r32.noise]).numpy()      # F.gumbel_softmax: -empty_like(logits).exponential_().log()
    out = {"meta/kind": np.array("maddpg"), "meta/F": np.int64(F), "meta/nb_agents": np.int64(N), "meta/shared": np.int64(shared),
           "meta/batch_size": np.int64(B), "meta/training_step": np.int64(nb_updates), "meta/gamma": np.float64(prop["gamma"]),
           "meta/soft_tau": np.float64(prop["soft_tau"]), "meta/gumbel_tau": np.float64(prop["gumbel_softmax_tau"]),
           "meta/lr_actor": np.float64(prop["lr_actor"]), "meta/lr_critic": np.float64(prop["lr_critic"]),
           "in/state": d["state"], "in/next_state": d["next_state"], "in/action": d["action"], "in/reward": d["reward"],
           "draws/index": np.array(r32.draws, dtype=np.int64).reshape(nb_updates, N, B),
           # per update and agent a: the N target picks in agent order, then the actor's own draw (ddpg.py:282-284, 331)
           "draws/noise": noise.reshape(nb_updates, N, N + 1, B, 2).transpose(0, 1, 3, 2, 4).copy()}
    names = [n for a in range(N) for n in ("critic%d" % a, "actor%d" % a)]      # the order of the backward() calls of one update
    _pack(out, (r32, r64), init, names)
    for name, g in r32.first_grads.items():      # the reference's float32 gradient too: its distance to ref64 is the actors' yardstick
        out["ref32/grad/%s" % name] = g.astype(np.float32)
    return out


# -- TarMAC-PPO -----------------------------------------------------------------------------------------------------------------------
def _run_tarmac(cfg, N, F, data, done, double, replay, seed):
    import torch
    ref_harness.load_reference()
    import agents.tarmac_ppo as module
    learner = _quiet(module.TarMAC_PPO, cfg, SimpleNamespace(net_seed=seed, no_wandb=True), num_state=F)
    learner.actor_net = _load(learner.actor_net, data["actor"], double)
    learner.critic_net = _load(learner.critic_net, data["critic"], double)
    learner.actor_optimizer = torch.optim.Adam(learner.actor_net.parameters(), learner.lr_actor)
    learner.critic_net_optimizer = torch.optim.Adam(learner.critic_net.parameters(), learner.lr_critic)
    T = data["action"].shape[0]
    for t in range(T):      # train_tarmacPPO.py:90-101: every agent's transition of a step, one flag for the step
        for a in range(N):
            learner.store_transition(PPOTransition(state=data["state"][t, a], action=[int(data["action"][t, a])],
                                                   a_log_prob=[float(data["a_prob"][t, a])], reward=float(data["reward"][t, a]),
                                                   next_state=data["state"][t + 1, a], done=bool(done[t, a])), a)
    run = _Run(replay)
    nets = {"actor": learner.actor_net, "critic": learner.critic_net}
    steps = [0]

    def after_critic_step(optimizer, args, kwargs):
        steps[0] += 1
        if steps[0] == 1:
            run.snapshot("first", nets)

    learner.critic_net_optimizer.register_step_post_hook(after_critic_step)
    run.bootstrap = np.zeros((T, N), dtype=np.float64)
    dtype = torch.float64 if double else torch.float32
    for t in range(T):      # agents/tarmac_ppo.py:137-138, before the update moves the critic
        if done[t, 0]:
            run.bootstrap[t] = learner.get_value(torch.tensor(data["state"][t + 1], dtype=dtype)).double().numpy().reshape(N)
    torch.manual_seed(seed + 77)
    with _instrumented(run, module, nets, double):
        learner.update(0)
    run.snapshot("last", nets)
    run.training_step = int(learner.training_step)
    return run


def make_tarmac(case, seed):
    """One hop, 'neighbours', no defects, the smallest shape ``tarmac_ppo.supported`` and ``critic_supported`` take: two agents, one
    sender, one feature, hidden state, key and value of 4, a critic of 4 hidden units; 12 env-steps."""
    import torch
    from tests import tarmac_critic_ref as tc
    N, c, F, H, K, V, Hc, T = 2, 1, 1, 4, 4, 4, 4, 12
    cfg = _config("TarMAC_PPO_prop", actor_hidden_state_size=H, communication_size=V, key_size=K, comm_num_hops=1, critic_hidden_layer_size=Hc,
                  with_gru=False, with_comm=True, number_agents_comm_tarmac=c, tarmac_comm_mode="neighbours", tarmac_comm_defect_prob=0,
                  batch_size=5, ppo_update_time=2)
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    ref_harness.load_reference()
    from agents.network import TarMAC_Actor
    torch.manual_seed(3000 + seed)
    g = torch.Generator(device="cpu").manual_seed(4000 + seed)
    actor = _quiet(TarMAC_Actor, num_obs=F, num_key=K, num_value=V, hidden_state_size=H, num_action=2, number_agents_comm=c,
                   comm_mode="neighbours", device=torch.device("cpu"), comm_defect_prob=0, num_hops=1, with_gru=False, with_comm=True)
    with torch.no_grad():      # as tests/golden/make_tarmac_golden.py: the default init leaves the probabilities at 0.33-0.67
        for pname, p in actor.named_parameters():
            if pname.endswith("weight"):
                p.mul_(2.0)
            else:
                p.uniform_(-0.5, 0.5, generator=g)
    dc = tc.draw(N, F, Hc, rows=T + 1, seed=seed)      # the critic and the states on tarmac_critic_ref's grids
    state = np.array(dc["state"])
    r = np.random.default_rng([seed, 0x7A3, N, F, T])
    action = r.integers(0, 2, (T, N)).astype(np.int64)
    reward = r.standard_normal((T, N)).astype(np.float32)
    with torch.no_grad():
        p = copy.deepcopy(actor).double()(torch.from_numpy(state[:T]).double()).gather(2, torch.from_numpy(action).unsqueeze(2)).squeeze(2).numpy()
    old = np.clip(p * r.uniform(0.7, 1.4, (T, N)), 0.02 + 1e-6, 0.98).astype(np.float32)
    data = dict(state=state, action=action, reward=reward, a_prob=old,
                actor={k: v.detach().numpy().astype(np.float32) for k, v in actor.state_dict().items()},
                critic={"critic.%d.%s" % (2 * i, w): np.array(dc[g_ + str(i + 1)], dtype=np.float32)
                        for i in range(3) for w, g_ in (("weight", "W"), ("bias", "b"))})
    done = np.zeros((T, N), dtype=bool)
    done[T - 1] = True
    r32 = _run_tarmac(cfg, N, F, data, done, False, None, seed)
    r64 = _run_tarmac(cfg, N, F, data, done, True, r32, seed)
    out = _ppo_out(cfg["TarMAC_PPO_prop"], "tarmac", F, N, T, N, 0, data, done, (r32, r64))
    out.update({"meta/c": np.int64(c), "meta/H": np.int64(H), "meta/K": np.int64(K), "meta/V": np.int64(V), "meta/Hc": np.int64(Hc)})
    out["meta/actor_grad_names"] = np.array([n for n, p_ in actor.named_parameters() if not n.startswith("comm.msg_state2state")])
    for name, g_ in r32.first_grads.items():      # the reference's float32 gradient: tarmac_ppo_ref's yardstick is its distance to fp64
        out["ref32/grad/%s" % name] = g_.astype(np.float32)
    return out


# -- the cases ------------------------------------------------------------------------------------------------------------------------
def _first_seed(make, case):
    """The case from the first data seed whose fixture meets every condition of tests/learner_golden.py ``conditions``."""
    from tests import learner_golden as lg
    why = None
    for seed in range(20):
        out = make(seed)
        out["meta/data_seed"] = np.int64(seed)
        try:
            lg.conditions(lg.Fixture(case, out))
            return out
        except AssertionError as e:
            why = e
    raise RuntimeError("%s: no data seed below 20 meets the conditions (%s)" % (case, why))


def generate(case: str) -> dict:
    """Run the reference for ``case`` -> the fixture's arrays."""
    if not ref_harness.available():
        raise RuntimeError("the reference is not present")
    cwd = os.getcwd()
    try:
        if case == "ppo_f51":
            return _first_seed(lambda s: make_ppo(case, 51, False, s), case)
        if case == "ppo_f21_zero":
            return _first_seed(lambda s: make_ppo(case, 21, True, s), case)
        if case == "mappo":
            return _first_seed(lambda s: make_mappo(case, s), case)
        if case == "dqn":
            return _first_seed(lambda s: make_dqn(case, False, 24, 1.0, s), case)
        if case == "dqn_clamped":
            return _first_seed(lambda s: make_dqn(case, False, 24, 20.0, s, w3_scale=8.0), case)
        if case == "ddqn_b1":
            return _first_seed(lambda s: make_dqn(case, True, 1, 1.0, s), case)
        if case == "maddpg_agents":
            return _first_seed(lambda s: make_maddpg(case, False, s), case)
        if case == "maddpg_shared":
            return _first_seed(lambda s: make_maddpg(case, True, s), case)
        if case == "tarmac_ppo":
            return _first_seed(lambda s: make_tarmac(case, s), case)
        raise KeyError(case)
    finally:
        os.chdir(cwd)      # ref_harness changes into the reference's root
