"""Adam on the GPU from a gradient on the GPU (include/mdr_policy.h: mdr_adam_step).

What every learner does with the gradient its kernels leave - ``clip_grad_norm_`` (DQN: an elementwise clamp), ``optimizer.step()``
(torch's Adam: nine ``multi_tensor_apply`` launches over 6-20 tensors) and, in DQN, the target blend - as ONE launch of
csrc/mdr_optim.hip: ``FusedAdam`` is a ``torch.optim.Optimizer`` that drops into the ``optimizer=`` hook of ``PPOLearner``,
``MAPPOLearner``, ``TarMACPPOLearner`` and ``DQNLearner``.  It is opt-in: the learners' default stays ``torch.optim.Adam``.

Parameters, gradients and targets stay where torch holds them: the kernel takes a table of {param, grad, target, count} segments,
so the gradients may be slices of a flat buffer (the gradient kernels') or autograd's own tensors.  The two moments are flat
buffers owned by the optimiser; ``state[p]["exp_avg"]`` / ``["exp_avg_sq"]`` are views of them, so ``state_dict()`` and
``load_state_dict()`` interchange with ``torch.optim.Adam``'s.

One visible difference from ``clip_grad_norm_`` + ``Adam.step()``: the gradient is never written.  After ``step(max_grad_norm=...)``
``p.grad`` still holds the unclipped gradient (``clip_grad_norm_`` scales ``.grad`` in place).

``step_nets`` steps a LIST of ``FusedAdam`` instances - the N critics or the N actors of MADDPG's per-agent networks - in at most two
launches (mdr_adam_step_nets), every net with its own norm, clip and blend and with the bits of its own ``step``.
"""
from __future__ import annotations

import ctypes as C
import math
import weakref
from typing import List, Optional, Sequence

import torch

from . import _native as nat

MAX_TENSORS = nat.MDR_ADAM_MAX_SEGMENTS


def _refusal(params: Sequence[torch.Tensor]) -> Optional[str]:
    """Why the kernel does not take these parameters (None: it does)."""
    params = list(params)
    if not params:
        return "no parameters"
    if len(params) > MAX_TENSORS:
        return "%d tensors: the kernel's segment table holds at most %d" % (len(params), MAX_TENSORS)
    for p in params:
        if not isinstance(p, torch.Tensor):
            return "parameters must be tensors"
        if p.dtype != torch.float32:
            return "parameters must be float32 (got %s)" % str(p.dtype).replace("torch.", "")
        if not p.is_contiguous():
            return "parameters must be contiguous"
    for p in params:
        if not p.is_cuda:
            return "parameters must be on the GPU (got a %s tensor)" % p.device.type
        if p.device != params[0].device:
            return "parameters must be on one GPU (got %s and %s)" % (params[0].device, p.device)
    return None


def supported(params) -> bool:
    """Does the kernel take these parameters?  At most 32 contiguous float32 tensors on one GPU."""
    return _refusal(list(params)) is None


class FusedAdam(torch.optim.Optimizer):
    """``torch.optim.Adam`` with its defaults other than ``lr``, ``betas`` and ``eps`` (no weight decay, no amsgrad, no maximize), one
    param group, at most 32 contiguous float32 tensors on one GPU; anything else raises ``ValueError``.  ``FusedAdam(params, lr)`` is the
    call the learners' ``optimizer=`` hook makes.

    ``max_fused_floats``: up to this many parameters in all the clipped step is one launch, above it two (0: the library's measured
    default, profiles/optim_step_README.md); both forms give the same bits."""

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, max_fused_floats: int = 0):
        if not 0.0 <= float(lr):
            raise ValueError("FusedAdam: invalid learning rate %r" % (lr,))
        if not (0.0 <= float(betas[0]) < 1.0 and 0.0 <= float(betas[1]) < 1.0):
            raise ValueError("FusedAdam: betas must lie in [0, 1), got %r" % (betas,))
        if not 0.0 <= float(eps):
            raise ValueError("FusedAdam: invalid eps %r" % (eps,))
        if int(max_fused_floats) < 0:
            raise ValueError("FusedAdam: max_fused_floats must be >= 0 (0: the library's default)")
        # the param group carries torch.optim.Adam's own keys (this torch's), so that either optimiser loads the other's state_dict
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults)
        defaults.update(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps))
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError("FusedAdam: one param group only (got %d)" % len(self.param_groups))
        self._params: List[torch.Tensor] = list(self.param_groups[0]["params"])
        why = _refusal(self._params)
        if why:
            raise ValueError("FusedAdam: " + why)
        self.max_fused_floats = int(max_fused_floats)
        dev = self._params[0].device
        self._device = dev
        self._counts = [p.numel() for p in self._params]
        total = sum(self._counts)
        self._exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self._exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self._m_views, self._v_views, off = [], [], 0
        for p, n in zip(self._params, self._counts):
            self._m_views.append(self._exp_avg[off:off + n].view_as(p))
            self._v_views.append(self._exp_avg_sq[off:off + n].view_as(p))
            off += n
        self._lib = nat.load()
        self._workspace = torch.empty(max(int(self._lib.mdr_adam_workspace_bytes(total)), 16), dtype=torch.uint8, device=dev)
        self._norm = torch.zeros((), dtype=torch.float32, device=dev)
        self._table = nat.MdrAdamSegments()
        self._table.struct_size = C.sizeof(nat.MdrAdamSegments)
        self._table.nb_segments = len(self._params)
        self._key = None      # the pointers the table was built from
        self._live: List[int] = []
        self._steps: List[torch.Tensor] = []
        self._t = 0      # the step count of the live parameters

    # -- state ---------------------------------------------------------------------------------------------------------------------
    def _adopt(self, i: int, step: Optional[torch.Tensor] = None) -> dict:
        """``state[p]`` of parameter i as views of the flat moments (created on its first gradient, as torch.optim.Adam does)."""
        p = self._params[i]
        st = self.state[p]
        st["step"] = step if step is not None else torch.tensor(0.0, dtype=torch.float32)
        st["exp_avg"], st["exp_avg_sq"] = self._m_views[i], self._v_views[i]
        return st

    def load_state_dict(self, state_dict) -> None:
        """``torch.optim.Adam``'s (or this class's) ``state_dict()``: the moments are copied into the flat buffers."""
        super().load_state_dict(state_dict)
        now = self.param_groups[0]["params"] if len(self.param_groups) == 1 else []
        if len(now) != len(self._params) or any(a is not b for a, b in zip(now, self._params)):
            raise ValueError("FusedAdam.load_state_dict: one param group over the same parameters")
        for i, p in enumerate(self._params):
            st = self.state.get(p)
            if not st:
                self._m_views[i].zero_()
                self._v_views[i].zero_()
                continue
            if "max_exp_avg_sq" in st:
                raise ValueError("FusedAdam.load_state_dict: amsgrad state is not supported")
            self._m_views[i].copy_(st["exp_avg"])
            self._v_views[i].copy_(st["exp_avg_sq"])
            step = torch.as_tensor(st["step"]).detach().to(device="cpu", dtype=torch.float32).reshape(()).clone()
            self._adopt(i, step)
        self._key = None

    def _check_group(self) -> dict:
        g = self.param_groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("FusedAdam: weight_decay, amsgrad and maximize are not offered")
        return g

    # -- the step ------------------------------------------------------------------------------------------------------------------
    def _build(self, key, grads, target) -> None:
        seg = self._table.seg
        self._live = []
        for i, p in enumerate(self._params):
            g = grads[i]
            if g is not None:
                if not g.is_cuda or g.device != self._device or g.dtype != torch.float32 or g.shape != p.shape or not g.is_contiguous():
                    raise ValueError("FusedAdam.step: gradients must be contiguous float32 tensors of the parameter's shape on its GPU")
                self._live.append(i)
            seg[i].param, seg[i].grad, seg[i].count = key[3 * i], key[3 * i + 1] or None, self._counts[i]
            seg[i].target = key[3 * i + 2] or None
        if target is not None:
            for p, t in zip(self._params, target):
                if t is not None and (t.device != self._device or t.dtype != torch.float32 or t.shape != p.shape or not t.is_contiguous()):
                    raise ValueError("FusedAdam.step: targets must be contiguous float32 tensors of the parameter's shape on its GPU")
        self._steps = [(self.state[self._params[i]] or self._adopt(i))["step"] for i in self._live]
        counts = {int(s) for s in self._steps}      # host tensors: read here, once per table, and mirrored in self._t
        if len(counts) > 1:
            raise ValueError("FusedAdam.step: the parameters are at different step counts (one launch takes one bias correction)")
        self._t = counts.pop() if counts else 0
        self._key = key

    def _table_key(self, target, blend: bool) -> list:
        """The pointers the segment table stands for - parameter, gradient, target of every tensor; autograd reallocates ``.grad``, so
        the table is rebuilt only when one of them moved (``step`` and ``step_nets``)."""
        grads = [p.grad for p in self._params]
        key = []
        for i, p in enumerate(self._params):
            g = grads[i]
            t = target[i] if blend else None
            key += [p.data_ptr(), g.data_ptr() if g is not None else 0, t.data_ptr() if t is not None else 0]
        if key != self._key:
            self._build(key, grads, target if blend else None)
        return key

    @torch.no_grad()
    def step(self, max_grad_norm: Optional[float] = None, grad_clamp: Optional[float] = None, target: Optional[Sequence[torch.Tensor]] = None,
             tau: Optional[float] = None, want_norm: bool = False, *, corrections: Optional[torch.Tensor] = None, slot: Optional[int] = None,
             base_dev: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """clamp -> norm clip -> Adam -> blend for every parameter that has a gradient, in one launch on the current stream; never
        synchronises.  ``max_grad_norm``: ``clip_grad_norm_``'s (None: no clip); ``grad_clamp``: ``p.grad.clamp_(-c, c)`` first (None: no
        clamp); ``target`` (tensors parallel to the parameters) with ``tau``: ``target = (1 - tau) target + tau p`` from the new p.
        ``p.grad`` is NOT modified (module docstring).  -> the total norm of the (clamped) gradient, a 0-dim device tensor overwritten
        by the next call, with ``want_norm``; None otherwise.

        ``corrections`` (float32 device tensor of ``correction_table`` pairs) with ``slot`` [and ``base_dev``, one device int32]: the
        launch a captured graph replays (mdr_adam_step_table) - the bias corrections are pair ``slot + base_dev`` of the table, read on
        the device, the host's step counts are neither read nor advanced (``advance`` does that after the replays), and the bits are
        those of the plain call at the step the pair was made for."""
        group = self._check_group()
        if corrections is not None or slot is not None or base_dev is not None:
            return self._step_table(group, max_grad_norm, grad_clamp, target, tau, want_norm, corrections, slot, base_dev)
        blend = target is not None and tau is not None and float(tau) > 0.0
        if (target is None) != (tau is None):
            raise ValueError("FusedAdam.step: target and tau go together")
        if blend and len(target) != len(self._params):
            raise ValueError("FusedAdam.step: target must list one tensor per parameter (%d), got %d" % (len(self._params), len(target)))
        self._table_key(target, blend)
        if not self._live:
            return self._norm.zero_() if want_norm else None
        t = self._t + 1
        beta1, beta2 = group["betas"]
        dev = self._device
        with torch.cuda.device(dev):
            rc = self._lib.mdr_adam_step(C.byref(self._table), self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(), float(group["lr"]), float(beta1),
                                         float(beta2), float(group["eps"]), t, float(max_grad_norm) if max_grad_norm is not None else 0.0,
                                         float(grad_clamp) if grad_clamp is not None else math.inf, float(tau) if blend else 0.0,
                                         self._workspace.data_ptr(), self._norm.data_ptr() if want_norm else None, self.max_fused_floats,
                                         torch.cuda.current_stream(dev).cuda_stream)
        nat.check(self._lib, None, rc, "mdr_adam_step")
        self._t = t
        torch._foreach_add_(self._steps, 1)      # host tensors, as torch.optim.Adam keeps them
        return self._norm if want_norm else None

    # -- the step a captured graph replays -----------------------------------------------------------------------------------------
    def _step_table(self, group, max_grad_norm, grad_clamp, target, tau, want_norm, corrections, slot, base_dev):
        if corrections is None or slot is None:
            raise ValueError("FusedAdam.step: corrections and slot go together (base_dev is optional)")
        dev = self._device
        if corrections.dtype != torch.float32 or corrections.device != dev or not corrections.is_contiguous() or corrections.numel() % 2:
            raise ValueError("FusedAdam.step: corrections must be a contiguous float32 tensor of {step_size, bc2_sqrt} pairs on the parameters' GPU")
        if not 0 <= int(slot) < corrections.numel() // 2:
            raise ValueError("FusedAdam.step: slot %r outside the table of %d pairs" % (slot, corrections.numel() // 2))
        if base_dev is not None and (base_dev.dtype != torch.int32 or base_dev.device != dev or base_dev.numel() != 1):
            raise ValueError("FusedAdam.step: base_dev must be one int32 on the parameters' GPU")
        blend = target is not None and tau is not None and float(tau) > 0.0
        if (target is None) != (tau is None):
            raise ValueError("FusedAdam.step: target and tau go together")
        if blend and len(target) != len(self._params):
            raise ValueError("FusedAdam.step: target must list one tensor per parameter (%d), got %d" % (len(self._params), len(target)))
        self._table_key(target, blend)
        if not self._live:
            return self._norm.zero_() if want_norm else None
        beta1, beta2 = group["betas"]
        with torch.cuda.device(dev):
            rc = self._lib.mdr_adam_step_table(C.byref(self._table), self._exp_avg.data_ptr(), self._exp_avg_sq.data_ptr(), float(group["lr"]),
                                               float(beta1), float(beta2), float(group["eps"]), corrections.data_ptr(), int(slot),
                                               base_dev.data_ptr() if base_dev is not None else None,
                                               float(max_grad_norm) if max_grad_norm is not None else 0.0,
                                               float(grad_clamp) if grad_clamp is not None else math.inf, float(tau) if blend else 0.0,
                                               self._workspace.data_ptr(), self._norm.data_ptr() if want_norm else None, self.max_fused_floats,
                                               torch.cuda.current_stream(dev).cuda_stream)
        nat.check(self._lib, None, rc, "mdr_adam_step_table")
        return self._norm if want_norm else None

    def step_count(self) -> int:
        """The step count of the parameters that have stepped (0: none has), from the host's bookkeeping; ValueError where they differ."""
        counts = {int(st["step"]) for st in (self.state.get(p) for p in self._params) if st}
        if len(counts) > 1:
            raise ValueError("FusedAdam: the parameters are at different step counts")
        return counts.pop() if counts else 0

    def correction_table(self, count: int, first_step: Optional[int] = None) -> torch.Tensor:
        """The {step_size, bc2_sqrt} pairs of the steps ``first_step`` (default: the next one) .. ``first_step + count - 1`` as a fresh
        pinned float32 [2 count] host tensor (mdr_adam_corrections: ``mdr_adam_step``'s own expressions, hence its bits).  A fresh
        tensor per call, so that a stream-ordered upload that has not run yet never sees a later call's values."""
        group = self._check_group()
        first = self.step_count() + 1 if first_step is None else int(first_step)
        out = torch.empty(2 * int(count), dtype=torch.float32, pin_memory=torch.cuda.is_available())
        beta1, beta2 = group["betas"]
        rc = self._lib.mdr_adam_corrections(float(group["lr"]), float(beta1), float(beta2), first, int(count), out.data_ptr())
        nat.check(self._lib, None, rc, "mdr_adam_corrections")
        return out

    def advance(self, count: int) -> None:
        """Add ``count`` to the step bookkeeping of every parameter that has a gradient - what ``count`` replayed table steps did on
        the device.  Host only."""
        if int(count) < 0:
            raise ValueError("FusedAdam.advance: count must be >= 0")
        steps = [(self.state[p] or self._adopt(i))["step"] for i, p in enumerate(self._params) if p.grad is not None]
        if steps:
            torch._foreach_add_(steps, int(count))
        self._t += int(count)


# -- N optimisers in one step ---------------------------------------------------------------------------------------------------------
class _NetsPlan:
    """What ``step_nets`` keeps for one list of optimisers: the device table of their segment records (mdr_adam_nets_bind), the
    workspace of their chunk sums, their norms, and the pointers every record was bound from."""

    def __init__(self, optimizers):
        lib, dev, n = nat.load(), optimizers[0]._device, len(optimizers)
        self.max_floats = max(sum(o._counts) for o in optimizers)
        self.table = torch.empty(max(int(lib.mdr_adam_nets_table_bytes(n)), 16), dtype=torch.uint8, device=dev)
        self.workspace = torch.empty(max(n * int(lib.mdr_adam_workspace_bytes(self.max_floats)), 16), dtype=torch.uint8, device=dev)
        self.norms = torch.zeros(n, dtype=torch.float32, device=dev)
        self.bound = [None] * n
        self.refs = [weakref.ref(o) for o in optimizers]      # an id may be taken again by a later object


def nets_refusal(optimizers) -> Optional[str]:
    """Why ``step_nets`` does not take these optimisers together (None: it does).  Decided on the host."""
    optimizers = list(optimizers)
    if not optimizers:
        return "no optimisers"
    if not all(isinstance(o, FusedAdam) for o in optimizers):
        return "every optimiser must be a FusedAdam"
    if len(set(map(id, optimizers))) != len(optimizers):
        return "an optimiser is listed twice"
    first = optimizers[0]
    g0 = first.param_groups[0]
    for o in optimizers:
        g = o._check_group()
        if o._device != first._device:
            return "the optimisers' parameters are on different GPUs"
        if float(g["lr"]) != float(g0["lr"]) or tuple(g["betas"]) != tuple(g0["betas"]) or float(g["eps"]) != float(g0["eps"]):
            return "lr, betas and eps must be the same for every optimiser (one launch takes one set)"
    if len({o.step_count() for o in optimizers}) > 1:
        return "the optimisers are at different step counts (one launch takes one bias correction)"
    return None


@torch.no_grad()
def step_nets(optimizers: Sequence[FusedAdam], max_grad_norm: Optional[float] = None, targets=None, tau: float = 0.0,
              want_norm: bool = False) -> Optional[torch.Tensor]:
    """``opt.step(max_grad_norm, target=targets[i], tau=tau)`` for every ``FusedAdam`` of ``optimizers`` in at most two
    launches (mdr_adam_step_nets): every net takes its own total norm, its own clip and its own blend, and its parameters, moments
    and targets end with the bits ``step`` gives.  The optimisers' own moment buffers are stepped and their own step counts advanced,
    so ``state_dict()`` does not know which form ran and a caller may change between the two at any step.  ``targets``: one list of
    tensors per optimiser, with ``tau`` > 0 (None: no blend).  ValueError (``nets_refusal``) where lr, betas, eps or the step counts
    differ between the optimisers: the caller then steps them one by one.  -> the N total norms (a float32 [N] device tensor
    overwritten by the next call) with ``want_norm``; None otherwise.  Never synchronises."""
    optimizers = list(optimizers)
    why = nets_refusal(optimizers)
    if why:
        raise ValueError("step_nets: " + why)
    blend = targets is not None and float(tau) > 0.0
    if targets is not None and len(targets) != len(optimizers):
        raise ValueError("step_nets: targets must list one sequence of tensors per optimiser")
    for i, o in enumerate(optimizers):
        if blend and len(targets[i]) != len(o._params):
            raise ValueError("step_nets: targets[%d] must list one tensor per parameter" % i)
    first = optimizers[0]
    plans = first.__dict__.setdefault("_nets_plans", {})
    ids = tuple(map(id, optimizers))
    plan = plans.get(ids)
    if plan is None or any(r() is not o for r, o in zip(plan.refs, optimizers)):
        plan = plans[ids] = _NetsPlan(optimizers)
    lib, dev = first._lib, first._device
    keys = [o._table_key(targets[i] if blend else None, blend) for i, o in enumerate(optimizers)]
    live = [o for o in optimizers if o._live]
    if len({o._t for o in live}) > 1:
        raise ValueError("step_nets: the optimisers are at different step counts (one launch takes one bias correction)")
    group = first.param_groups[0]
    beta1, beta2 = group["betas"]
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream(dev).cuda_stream
        for i, o in enumerate(optimizers):      # a record is bound again only when one of its pointers moved
            if plan.bound[i] != keys[i]:
                rc = lib.mdr_adam_nets_bind(plan.table.data_ptr(), i, C.byref(o._table), o._exp_avg.data_ptr(), o._exp_avg_sq.data_ptr(), st)
                nat.check(lib, None, rc, "mdr_adam_nets_bind")
                plan.bound[i] = list(keys[i])
        if live:
            rc = lib.mdr_adam_step_nets(plan.table.data_ptr(), len(optimizers), plan.max_floats, float(group["lr"]), float(beta1), float(beta2),
                                        float(group["eps"]), live[0]._t + 1, float(max_grad_norm) if max_grad_norm is not None else 0.0,
                                        math.inf, float(tau) if blend else 0.0, plan.workspace.data_ptr(), plan.norms.data_ptr() if want_norm else None, st)
            nat.check(lib, None, rc, "mdr_adam_step_nets")
    for o in live:
        o._t += 1
        torch._foreach_add_(o._steps, 1)
    if not want_norm:
        return None
    return plan.norms if live else plan.norms.zero_()
