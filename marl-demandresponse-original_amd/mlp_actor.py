"""Acting with an actor of up to 256 hidden units per layer in one HIP kernel (include/mdr_policy.h: mdr_mlp_actor_sample).

MADDPG is the reference's default trainer (cli.py:38, agents/ddpg.py, train_ddpg.py) and its actor has two hidden layers of 256 units
(config.py ``DDPG_prop.actor_hidden_dim``), beyond the 127 of ``FusedActor``.  ``FusedMLPActor`` runs observation rows -> Linear - ReLU -
Linear - ReLU - Linear(2) -> softmax -> draw or argmax for every agent in one launch (csrc/mdr_mlp_actor.hip): persistent workgroups keep
their slabs of W1 and W2 in registers and stride over tiles of 32 agents.  The weights are read from the module's own tensors on every
call - there is no packed copy - so an optimiser step between two calls is seen by the next one, which is what ``train_maddpg`` needs:
it changes the actor at every update.  Draws, outputs and ``step_dev`` are ``FusedActor.sample``'s, so ``deploy_policy`` takes a
``FusedMLPActor`` through its duck-typed branch.  Nothing on the call path synchronises with the host.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _learner as L
from . import _native as nat

MAX_STATE, MAX_HIDDEN = 128, 256      # the kernel's limits (include/mdr_policy.h: mdr_mlp_actor_sample)
PRECISIONS = {"fp32": "mdr_mlp_actor_sample", "bf16x3": "mdr_mlp_actor_sample_bf16x3"}      # precision -> entry point


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
