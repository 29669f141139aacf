"""Acting with an actor of up to 256 hidden units per layer in one HIP kernel (include/mdr_policy.h: mdr_mlp_actor_sample).

MADDPG is the reference's default trainer (cli.py:38, agents/ddpg.py, train_ddpg.py) and its actor has two hidden layers of 256 units
(config.py ``DDPG_prop.actor_hidden_dim``), beyond the 127 of ``FusedActor``.  ``FusedMLPActor`` runs observation rows -> Linear - ReLU -
Linear - ReLU - Linear(2) -> softmax -> draw or argmax for every agent in one launch (csrc/mdr_mlp_actor.hip): persistent workgroups keep
their slabs of W1 and W2 in registers and stride over tiles of 32 agents.  The weights are read from the module's own tensors on every
call - there is no packed copy - so an optimiser step between two calls is seen by the next one, which is what ``train_maddpg`` needs:
it changes the actor at every update.  Draws, outputs and ``step_dev`` are ``FusedActor.sample``'s, so ``deploy_policy`` takes a
``FusedMLPActor`` through its duck-typed branch.  Nothing on the call path synchronises with the host.
``FusedMLPActor.sample_env`` is observe -> act (mdr_env_mlp_actor_sample, csrc/mdr_mlp_actor_observe.hip): the same outputs, bit for
bit, from the env's compact state - no row kernel, no rows - for the default observation of 51 features; opt-in everywhere.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _learner as L
from . import _native as nat

MAX_STATE, MAX_HIDDEN = 128, 256      # the kernel's limits (include/mdr_policy.h: mdr_mlp_actor_sample)
PRECISIONS = {"fp32": "mdr_mlp_actor_sample", "bf16x3": "mdr_mlp_actor_sample_bf16x3"}      # precision -> entry point
OBSERVE_ENTRIES = {"fp32": "mdr_env_mlp_actor_sample", "bf16x3": "mdr_env_mlp_actor_sample_bf16x3"}      # ... of sample_env
OBSERVE_NUM_STATE = 51      # the default observation, which the observe forms build


def default_observation_refusal(env) -> Optional[str]:
    """Why observe -> act does not cover ``env`` (None: it does) - what ``mdr_env_mlp_actor_sample`` checks of the env, read on the
    host: the default observation of an unsharded env of at least 11 houses."""
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


class FusedMLPActor:
    """``module``: anything ``_learner.fc_layers`` resolves (``DDPGNetworkMLP``, ``ActorMLP``, the reference's nets) with at most 128
    input features, at most 256 units in each hidden layer (any size) and 2 outputs, float32 on the GPU.  The module is held, not
    copied.  ``greedy=True``: the argmax (the first maximum on ties) instead of a draw - ``DDPGAgent.act``.  ``precision``: "fp32"
    (default) - exact fp32 products; "bf16x3" - both hidden layers on the bf16 matrix cores with every operand split into a bf16 head
    and tail (``mdr_mlp_actor_sample_bf16x3``, csrc/mdr_mlp_actor_bf16.hip): probabilities within 2e-3 |p| + 2e-5 of fp64, the same
    nets, arguments and draw.  Measured: profiles/mlp_actor_bf16_README.md."""

    def __init__(self, module, greedy: bool = False, precision: str = "fp32"):
        if precision not in PRECISIONS:
            raise ValueError("FusedMLPActor: precision must be 'fp32' or 'bf16x3', not %r" % (precision,))
        why = self.refusal(module)
        if why:
            raise ValueError("FusedMLPActor: " + why)
        self.module, self.greedy, self.precision = module, bool(greedy), precision
        self._lib = nat.load()

    @staticmethod
    def refusal(module) -> Optional[str]:
        """Why the kernel does not take ``module`` (None: it does)."""
        fc = L.fc_layers(module)
        if fc is None:
            return "the kernel covers Linear-ReLU-Linear-ReLU-Linear (DDPGNetworkMLP, or an `fc` list of three biased Linear layers)"
        if fc[1].in_features != fc[0].out_features or fc[2].in_features != fc[1].out_features:
            return "the three layers do not chain"
        if fc[0].in_features > MAX_STATE:
            return "num_state = %d: the kernel covers at most %d input features" % (fc[0].in_features, MAX_STATE)
        if fc[0].out_features > MAX_HIDDEN or fc[1].out_features > MAX_HIDDEN:
            return "hidden layers of %d and %d units: the kernel covers at most %d" % (fc[0].out_features, fc[1].out_features, MAX_HIDDEN)
        if fc[2].out_features != 2:
            return "%d outputs: the kernel covers an actor of 2 actions" % fc[2].out_features
        if not all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in L.mlp_params(fc)):
            return "parameters must be contiguous float32 tensors on the GPU"
        return None

    @classmethod
    def supported(cls, module) -> bool:
        """Does the kernel take this net?  Three biased Linear layers, F <= 128, hidden layers <= 256 (any size), 2 actions, float32
        on the GPU."""
        return cls.refusal(module) is None

    @property
    def device(self) -> torch.device:
        return L.fc_layers(self.module)[0].weight.device

    @property
    def num_state(self) -> int:
        return L.fc_layers(self.module)[0].in_features

    def sample(self, rows: torch.Tensor, seed: int, step: int, step_dev: Optional[torch.Tensor] = None, greedy: Optional[bool] = None,
               action: Optional[torch.Tensor] = None, a_prob: Optional[torch.Tensor] = None, want_probs: bool = False,
               max_workgroups: int = 0) -> Tuple[torch.Tensor, ...]:
        """``rows`` float32 [A, F] on the device with unit inner stride and a row stride >= F -> (action uint8 [A], a_prob float32 [A]
        [, probs [A, 2]]), as ``FusedActor.sample``.  ``step_dev``: device int32 added to ``step`` inside the kernel
        (``env.device_time_index`` when the call is captured in a graph).  ``greedy``: None - the constructor's.  With ``action`` and
        ``a_prob`` given (and no ``want_probs``) nothing is allocated.  ``max_workgroups`` bounds the grid (0: the library's choice);
        the outputs do not depend on it."""
        why = self.refusal(self.module)      # the module is the caller's: it may have changed since the constructor looked
        if why:
            raise ValueError("FusedMLPActor.sample: " + why)
        fc = L.fc_layers(self.module)
        dev, _, ld, A = L.check_rows(fc, rows, None, "FusedMLPActor.sample")
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != dev):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        action = torch.empty(A, dtype=torch.uint8, device=dev) if action is None else L.whole(action, torch.uint8, A, dev, "FusedMLPActor.sample", "action")
        a_prob = torch.empty(A, dtype=torch.float32, device=dev) if a_prob is None else L.whole(a_prob, torch.float32, A, dev, "FusedMLPActor.sample", "a_prob")
        probs = torch.empty((A, 2), dtype=torch.float32, device=dev) if want_probs else None
        desc = L.mlp_desc(fc)
        entry = PRECISIONS[self.precision]
        with torch.cuda.device(dev):
            rc = getattr(self._lib, entry)(C.byref(desc), L.ptr(rows), ld, A, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                           C.c_uint64(int(step) & (2 ** 64 - 1)), L.ptr(step_dev),
                                           int(self.greedy if greedy is None else bool(greedy)), int(max_workgroups), L.ptr(action),
                                           L.ptr(a_prob), L.ptr(probs), L.stream(dev))
        nat.check(self._lib, None, rc, entry)
        return (action, a_prob, probs) if want_probs else (action, a_prob)

    def _observe_refusal(self, env) -> Optional[str]:
        """Why ``sample_env`` cannot serve ``env`` (None: it can): the net's input size, the env, then ``refusal`` of the net."""
        fc = L.fc_layers(self.module)
        if fc is not None and fc[0].in_features != OBSERVE_NUM_STATE:
            return "the actor takes %d features, observe -> act builds the default observation of %d" % (fc[0].in_features, OBSERVE_NUM_STATE)
        return default_observation_refusal(env) or self.refusal(self.module)

    def observe_supported(self, env) -> bool:
        """Can ``sample_env`` serve ``env``?  The default observation of 51 features (no optional state / message column, ten circular
        neighbours, no link defects) of an unsharded env of at least 11 houses, and a net ``sample`` takes with ``num_state == 51``.
        Decided on the host: nothing is launched."""
        return self._observe_refusal(env) is None

    def sample_env(self, env, seed: int, step: int, step_dev: Optional[torch.Tensor] = None, greedy: Optional[bool] = None,
                   action: Optional[torch.Tensor] = None, a_prob: Optional[torch.Tensor] = None, want_probs: bool = False,
                   rows_out: Optional[torch.Tensor] = None, max_workgroups: int = 0) -> Tuple[torch.Tensor, ...]:
        """Observe -> act (``mdr_env_mlp_actor_sample``, ``_bf16x3`` with ``precision="bf16x3"``; csrc/mdr_mlp_actor_observe.hip):
        ``sample(env.obs_vector("rows").view(E * N, 51), ...)`` without the rows - no row kernel, no row read; the kernel builds the 51
        features of its tile of agents in LDS from the env's compact state.  Returns what ``sample`` returns, bit for bit, every
        argument as there.  ``rows_out`` (float32, contiguous, A * 51 elements, on the env's device): also receives the rows, bit for
        bit ``env.obs_vector("rows")`` (the transition buffer's ``state``).  ``ValueError`` before any launch for an env or net it
        does not cover (``observe_supported``).  With ``action`` and ``a_prob`` given (and no ``want_probs``) nothing is allocated.
        Measured against rows + ``sample``: profiles/mlp_actor_observe_README.md."""
        what = "FusedMLPActor.sample_env"
        why = self._observe_refusal(env)
        if why:
            raise ValueError("%s: %s" % (what, why))
        fc = L.fc_layers(self.module)
        dev = env.device
        if dev != fc[0].weight.device:
            raise ValueError("%s: the env and the actor's parameters must be on the same device" % what)
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != dev):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        A = env.nb_envs * env.nb_houses
        action = torch.empty(A, dtype=torch.uint8, device=dev) if action is None else L.whole(action, torch.uint8, A, dev, what, "action")
        a_prob = torch.empty(A, dtype=torch.float32, device=dev) if a_prob is None else L.whole(a_prob, torch.float32, A, dev, what, "a_prob")
        if rows_out is not None:
            L.whole(rows_out, torch.float32, A * OBSERVE_NUM_STATE, dev, what, "rows_out")
        probs = torch.empty((A, 2), dtype=torch.float32, device=dev) if want_probs else None
        desc = L.mlp_desc(fc)
        spec = env._obs_spec("rows")
        entry = OBSERVE_ENTRIES[self.precision]
        with torch.cuda.device(dev):
            rc = getattr(self._lib, entry)(env._handle, C.byref(spec), C.byref(desc), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                           C.c_uint64(int(step) & (2 ** 64 - 1)), L.ptr(step_dev),
                                           int(self.greedy if greedy is None else bool(greedy)), int(max_workgroups), L.ptr(action),
                                           L.ptr(a_prob), L.ptr(probs), L.ptr(rows_out), L.stream(dev))
        if rc == nat.MDR_ERR_UNSUPPORTED:
            raise ValueError("%s: %s" % (what, self._lib.mdr_last_error(env._handle).decode()))
        nat.check(self._lib, env._handle, rc, entry)
        return (action, a_prob, probs) if want_probs else (action, a_prob)


class FusedMLPActors:
    """One actor per agent (MADDPG with unshared networks, ddpg.py:200-213) acting in ONE launch (include/mdr_policy.h:
    mdr_mlp_actors_sample): row ``e * N + k`` of the observation rows goes through ``modules[k]``.  ``modules``: a sequence of 1 to 32
    nets ``FusedMLPActor`` takes, all of one shape and on one device.  The modules are held, not copied, and their descriptors are
    rebuilt from the live tensors on every call, so every agent's optimiser step is seen by the next call.  The draw is keyed by the
    row's index in the whole batch: rows ``k::N`` have the bits ``FusedMLPActor(modules[k])`` gives them on the same batch."""

    def __init__(self, modules, greedy: bool = False):
        modules = list(modules)
        why = self.refusal(modules)
        if why:
            raise ValueError("FusedMLPActors: " + why)
        self.modules, self.greedy = modules, bool(greedy)
        self._lib = nat.load()

    @staticmethod
    def refusal(modules) -> Optional[str]:
        """Why the kernel does not take these nets (None: it does)."""
        modules = list(modules)
        if not 1 <= len(modules) <= nat.MDR_MAX_AGENT_NETS:
            return "%d nets: the kernel covers 1 to %d" % (len(modules), nat.MDR_MAX_AGENT_NETS)
        for k, m in enumerate(modules):
            why = FusedMLPActor.refusal(m)
            if why:
                return "net %d: %s" % (k, why)
        fcs = [L.fc_layers(m) for m in modules]
        shape = [lin.weight.shape for lin in fcs[0]]
        for k, fc in enumerate(fcs):
            if [lin.weight.shape for lin in fc] != shape:
                return "net %d has another shape than net 0: all nets share num_state and both hidden sizes" % k
            if fc[0].weight.device != fcs[0][0].weight.device:
                return "net %d is on another device than net 0" % k
        return None

    @classmethod
    def supported(cls, modules) -> bool:
        """Does the kernel take these nets?  1 to 32 of them, each one ``FusedMLPActor`` takes, of one shape, on one device."""
        return cls.refusal(modules) is None

    @property
    def device(self) -> torch.device:
        return L.fc_layers(self.modules[0])[0].weight.device

    @property
    def num_state(self) -> int:
        return L.fc_layers(self.modules[0])[0].in_features

    def sample(self, rows: torch.Tensor, seed: int, step: int, step_dev: Optional[torch.Tensor] = None, greedy: Optional[bool] = None,
               action: Optional[torch.Tensor] = None, a_prob: Optional[torch.Tensor] = None, want_probs: bool = False,
               max_workgroups: int = 0) -> Tuple[torch.Tensor, ...]:
        """``rows`` float32 [E * N, F] (env-major: row e N + k is agent k of env e) -> what ``FusedMLPActor.sample`` returns, every
        argument as there."""
        what = "FusedMLPActors.sample"
        why = self.refusal(self.modules)      # the modules are the caller's: they may have changed since the constructor looked
        if why:
            raise ValueError("%s: %s" % (what, why))
        fcs = [L.fc_layers(m) for m in self.modules]
        N = len(fcs)
        dev, _, ld, A = L.check_rows(fcs[0], rows, None, what)
        if A % N != 0:
            raise ValueError("%s: %d rows are no multiple of the %d nets" % (what, A, N))
        if step_dev is not None and (step_dev.dtype != torch.int32 or step_dev.device != dev):
            raise ValueError("step_dev must be an int32 tensor on the device (env.device_time_index)")
        action = torch.empty(A, dtype=torch.uint8, device=dev) if action is None else L.whole(action, torch.uint8, A, dev, what, "action")
        a_prob = torch.empty(A, dtype=torch.float32, device=dev) if a_prob is None else L.whole(a_prob, torch.float32, A, dev, what, "a_prob")
        probs = torch.empty((A, 2), dtype=torch.float32, device=dev) if want_probs else None
        descs = L.mlp_descs(fcs)
        with torch.cuda.device(dev):
            rc = self._lib.mdr_mlp_actors_sample(descs, N, L.ptr(rows), ld, A, C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                 C.c_uint64(int(step) & (2 ** 64 - 1)), L.ptr(step_dev),
                                                 int(self.greedy if greedy is None else bool(greedy)), int(max_workgroups), L.ptr(action),
                                                 L.ptr(a_prob), L.ptr(probs), L.stream(dev))
        nat.check(self._lib, None, rc, "mdr_mlp_actors_sample")
        return (action, a_prob, probs) if want_probs else (action, a_prob)
