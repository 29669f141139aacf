"""Device-side minibatch indices and the captured update of PPOLearner, MAPPOLearner and DQNLearner (csrc/mdr_minibatch.hip,
include/mdr_policy.h: mdr_minibatch_permutation, mdr_minibatch_sample, mdr_update_cursor_set, mdr_adam_step_table).

At the reference's sizes an update is host time: a PPO minibatch is six launches of 60-80 us of GPU work behind 190 us of Python,
ctypes and launch overhead (profiles/optim_step_README.md).  Three host-side things keep an update from being replayed as a graph -
the minibatch indices (``torch.randperm`` under a generator seeded per epoch), Adam's bias corrections (kernel arguments formed from
the host's step count) and host counters.  Here each has a device-side counterpart:

* ``permutation`` / ``sample``: the indices as a function of (seed, epoch or step, element) through Philox - ``sampler="philox"`` of
  the learners, eager launches, usable on its own;
* ``FusedAdam.step(corrections=, slot=, base_dev=)``: the bias corrections from a table in device memory;
* a block of int32 cursors (epoch, table base, the seed as the Philox key; DQN: the buffer's fill count and the step) that one-thread
  kernels set and advance.

``PPOUpdateGraph`` holds ONE epoch - the permutation, every minibatch's critic call, actor call and two table steps, the loss sums,
the cursor advance - as one ``torch.cuda.CUDAGraph`` captured on one side stream (a chain of nodes, no fork); an update copies the batch
into the graph's static input buffers, resets the cursors, uploads the corrections of all its steps and replays the graph
``ppo_update_time`` times.  ``DQNUpdateGraph`` holds one update.  Nothing is allocated inside a capture, and a capture leaves no
trace: kernels do not run while capturing, and the warm-up pass before it (first-use kernel attributes, the flat gradient buffers, the
optimiser's segment table) runs on a snapshot of parameters and moments that is restored.  The graphed update launches the same
kernels with the same arguments as the eager ``sampler="philox"`` update and gives the same bits.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _learner as L
from . import _native as nat
from .optim import FusedAdam


def _i32(x: int) -> int:
    """The low 32 bits of x as the int32 of the same bit pattern."""
    x = int(x) & 0xFFFFFFFF
    return x - (1 << 32) if x >= (1 << 31) else x


def _check_int32(t: Optional[torch.Tensor], dev, count: int, what: str) -> None:
    if t is not None and (t.dtype != torch.int32 or t.device != dev or t.numel() < count or not t.is_contiguous()):
        raise ValueError("%s must be a contiguous int32 tensor of at least %d elements on %s" % (what, count, dev))


def cursor_set(block: torch.Tensor, values: Sequence[int], offset: int = 0) -> None:
    """block[offset + k] = values[k] (1 to 4 int32 values, passed as kernel arguments) by a one-thread kernel on the current stream."""
    vals = [_i32(v) for v in values]
    if not 1 <= len(vals) <= 4:
        raise ValueError("cursor_set: 1 to 4 values")
    _check_int32(block, block.device, int(offset) + len(vals), "cursor_set: block")
    if offset < 0 or not block.is_cuda:
        raise ValueError("cursor_set: a device block and an offset >= 0")
    lib = nat.load()
    with torch.cuda.device(block.device):
        rc = lib.mdr_update_cursor_set(C.c_void_p(block.data_ptr() + 4 * int(offset)), len(vals), *(vals + [0] * (4 - len(vals))), L.stream(block.device))
    nat.check(lib, None, rc, "mdr_update_cursor_set")


def cursor_add(block: torch.Tensor, index: int, delta: int) -> None:
    """block[index] += delta by a one-thread kernel on the current stream."""
    _check_int32(block, block.device, int(index) + 1, "cursor_add: block")
    if index < 0 or not block.is_cuda:
        raise ValueError("cursor_add: a device block and an index >= 0")
    lib = nat.load()
    with torch.cuda.device(block.device):
        rc = lib.mdr_update_cursor_add(C.c_void_p(block.data_ptr()), int(index), _i32(delta), L.stream(block.device))
    nat.check(lib, None, rc, "mdr_update_cursor_add")


def _out(out: Optional[torch.Tensor], n: int, dev, what: str) -> torch.Tensor:
    if out is None:
        return torch.empty(int(n), dtype=torch.int64, device=dev)
    if out.dtype != torch.int64 or out.device != torch.device(dev) or out.numel() < n or not out.is_contiguous():
        raise ValueError("%s: out must be a contiguous int64 tensor of at least %d elements on %s" % (what, n, dev))
    return out


def permutation(n: int, seed: int, epoch: int, device, out: Optional[torch.Tensor] = None, cursor: Optional[torch.Tensor] = None,
                key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A permutation of 0 .. n - 1 (int64 [n] on ``device``; into ``out[:n]`` where given) drawn by (seed, epoch): the four-round
    Feistel network with cycle walking of include/mdr_policy.h, one launch on the current stream.  ``cursor``: one device int32 added
    to the low word of ``epoch`` when the kernel runs; ``key``: device int32 [2] = (seed lo, seed hi) read in place of ``seed``."""
    dev = torch.device(device)
    n = int(n)
    if n < 0:
        raise ValueError("permutation: n must be >= 0")
    res = _out(out, n, dev, "permutation")
    _check_int32(cursor, dev, 1, "permutation: cursor")
    _check_int32(key, dev, 2, "permutation: key")
    lib = nat.load()
    cur = C.c_void_p(cursor.data_ptr()) if cursor is not None else None
    with torch.cuda.device(dev):
        if key is not None:
            rc = lib.mdr_minibatch_permutation_keyed(n, C.c_void_p(key.data_ptr()), int(epoch) & (2 ** 64 - 1), cur, C.c_void_p(res.data_ptr()), L.stream(dev))
        else:
            rc = lib.mdr_minibatch_permutation(n, int(seed) & (2 ** 64 - 1), int(epoch) & (2 ** 64 - 1), cur, C.c_void_p(res.data_ptr()), L.stream(dev))
    nat.check(lib, None, rc, "mdr_minibatch_permutation")
    return res[:n] if out is not None else res


def sample(nb: int, length, seed: int, step: int, device, out: Optional[torch.Tensor] = None, cursor: Optional[torch.Tensor] = None,
           key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``nb`` positions drawn uniformly with replacement from [0, length) (int64 [nb] on ``device``) by (seed, step), as
    ``random.choices`` draws them (agents/buffer.py:26-27): (word * length) >> 32 of one Philox word per position, biased by at most
    length / 2^32.  ``length``: an int (1 .. 2^32 - 1) or one device int64 read when the kernel runs; ``cursor`` / ``key`` as
    ``permutation``'s (the cursor is added to the low word of ``step``)."""
    dev = torch.device(device)
    nb = int(nb)
    if nb < 0:
        raise ValueError("sample: nb must be >= 0")
    res = _out(out, nb, dev, "sample")
    _check_int32(cursor, dev, 1, "sample: cursor")
    _check_int32(key, dev, 2, "sample: key")
    len_dev, len_host = None, 0
    if isinstance(length, torch.Tensor):
        if length.dtype != torch.int64 or length.device != dev or length.numel() != 1:
            raise ValueError("sample: a device length must be one int64 on %s" % dev)
        len_dev = C.c_void_p(length.data_ptr())
    else:
        len_host = int(length)
        if not 1 <= len_host <= 2 ** 32 - 1:
            raise ValueError("sample: length must lie in [1, 2^32 - 1]")
    lib = nat.load()
    cur = C.c_void_p(cursor.data_ptr()) if cursor is not None else None
    with torch.cuda.device(dev):
        if key is not None:
            rc = lib.mdr_minibatch_sample_keyed(nb, len_dev, len_host, C.c_void_p(key.data_ptr()), int(step) & (2 ** 64 - 1), cur, C.c_void_p(res.data_ptr()),
                                                L.stream(dev))
        else:
            rc = lib.mdr_minibatch_sample(nb, len_dev, len_host, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), cur, C.c_void_p(res.data_ptr()),
                                          L.stream(dev))
    nat.check(lib, None, rc, "mdr_minibatch_sample")
    return res[:nb] if out is not None else res


# -- what a captured update needs of a learner ---------------------------------------------------------------------------------------
def refusal(backend: str, sampler: str, optimizers, uses_kernels: bool) -> Optional[str]:
    """Why ``graph=True`` is refused at construction (None: it is not)."""
    if backend == "torch":
        return "backend='torch' launches autograd's kernels, not a fixed chain"
    if sampler != "philox":
        return "sampler=%r draws the indices on the host; graph=True needs sampler='philox'" % (sampler,)
    if not all(isinstance(o, FusedAdam) for o in optimizers):
        return "optimizer=FusedAdam is required (the bias corrections must come from device memory)"
    if not uses_kernels:
        return "the kernels do not take these networks"
    return None


def _flat_grad(net, floats: int) -> torch.Tensor:
    """The flat gradient of ``net`` with the six ``p.grad`` rebound to views of it: the captured optimiser step reads them there."""
    params = L.mlp_params(L.fc_layers(net))
    flat = L.flat_grad(net, floats, params[0].device)
    L.publish(params, flat, L.REBIND)
    return flat


def _signature(nets) -> list:
    sig = []
    for net in nets:
        for p in L.mlp_params(L.fc_layers(net)):
            sig += [p.data_ptr(), p.grad.data_ptr() if p.grad is not None else 0]
    return sig


class _Snapshot:
    """Parameters, target parameters and moments before a warm-up pass; ``restore`` puts them back."""

    def __init__(self, tensors):
        self.tensors = list(tensors)
        self.clones = [t.detach().clone() for t in self.tensors]

    @torch.no_grad()
    def restore(self) -> None:
        for t, c in zip(self.tensors, self.clones):
            t.copy_(c)


def _capture(record, snapshot_tensors, dev) -> torch.cuda.CUDAGraph:
    """Warm-up pass of ``record`` on a side stream under a snapshot, then its capture on that stream."""
    side = torch.cuda.Stream(device=dev)
    snap = _Snapshot(snapshot_tensors)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        record()
        snap.restore()
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with nat.gc_paused(), torch.cuda.graph(graph, stream=side):
        record()
    return graph


class PPOUpdateGraph:
    """One epoch of ``PPOLearner.update`` / ``MAPPOLearner.update`` over a batch of T x A transitions of F features as one graph."""

    EPOCH, BASE, KEY = 0, 1, 2      # the cursor block: epoch, table base, key lo, key hi

    def __init__(self, learner, T: int, A: int, F: int):
        self.learner = learner
        dev = next(learner.actor.parameters()).device
        self.dev = dev
        self.n, self.F, self.bs, self.epochs = T * A, F, learner.batch_size, learner.ppo_update_time
        self.m = (self.n + self.bs - 1) // self.bs
        n = self.n
        self.state = torch.zeros((n, F), dtype=torch.float32, device=dev)
        self.action = torch.zeros(n, dtype=torch.int64, device=dev)
        self.a_prob = torch.ones(n, dtype=torch.float32, device=dev)
        self.ret = torch.zeros(n, dtype=torch.float32, device=dev)
        self.perm = torch.zeros(n, dtype=torch.int64, device=dev)
        self.block = torch.zeros(4, dtype=torch.int32, device=dev)
        self.a_table = torch.ones(2 * self.epochs * self.m, dtype=torch.float32, device=dev)
        self.c_table = torch.ones(2 * self.epochs * self.m, dtype=torch.float32, device=dev)
        self.a_sum = torch.zeros((), dtype=torch.float32, device=dev)
        self.c_sum = torch.zeros((), dtype=torch.float32, device=dev)
        self.a_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.c_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.value = torch.zeros(self.bs, dtype=torch.float32, device=dev)
        self.adv = torch.zeros(self.bs, dtype=torch.float32, device=dev)
        self.a_desc, self.c_desc = L.mlp_desc(L.fc_layers(learner.actor)), L.mlp_desc(L.fc_layers(learner.critic))
        # the learner's own calls (wide or narrow, MAPPO's joint critic), here on the graph's static buffers
        (a_sizes, self.actor_launch), (c_sizes, self.critic_launch) = learner._actor_kernel(), learner._critic_kernel()
        rows = {min(self.bs, n), n - (self.m - 1) * self.bs}      # a full minibatch and the tail
        a_floats, a_bytes = zip(*(a_sizes(self.a_desc, B) for B in rows))
        c_floats, c_bytes = zip(*(c_sizes(self.c_desc, B) for B in rows))
        self.workspace = torch.empty(max(16, *a_bytes, *c_bytes), dtype=torch.uint8, device=dev)      # the graph's own: the shared one may be reallocated
        self.a_flat, self.c_flat = _flat_grad(learner.actor, a_floats[0]), _flat_grad(learner.critic, c_floats[0])
        a_opt, c_opt = learner.actor_optimizer, learner.critic_optimizer
        held = list(learner.actor.parameters()) + list(learner.critic.parameters()) + [a_opt._exp_avg, a_opt._exp_avg_sq, c_opt._exp_avg, c_opt._exp_avg_sq]
        self.graph = _capture(self._record, held, dev)
        self.signature = _signature((learner.actor, learner.critic))

    def _record(self) -> None:
        """The launches of one epoch on the current stream, from the static buffers alone."""
        learner, dev = self.learner, self.dev
        st = L.stream(dev)
        base = self.block[self.BASE:self.BASE + 1]
        with torch.cuda.device(dev):
            permutation(self.n, 0, 0, dev, out=self.perm, cursor=self.block[self.EPOCH:], key=self.block[self.KEY:])
            for j in range(self.m):
                index = self.perm[j * self.bs:(j + 1) * self.bs]      # a view (the last one shorter): slicing launches nothing
                B = int(index.shape[0])
                self.critic_launch(self.c_desc, self.state, self.F, self.action, self.ret, index, B, self.workspace, self.c_flat, self.c_loss,
                                   self.value, self.adv, st)
                self.actor_launch(self.a_desc, self.state, self.F, self.action, self.a_prob, index, B, self.adv, self.workspace, self.a_flat,
                                  self.a_loss, None, st)
                for net, opt, table in ((learner.actor, learner.actor_optimizer, self.a_table), (learner.critic, learner.critic_optimizer, self.c_table)):
                    L.clip_and_step(opt, net.parameters(), learner.max_grad_norm, corrections=table, slot=j, base_dev=base)
                self.a_sum.add_(self.a_loss)
                self.c_sum.add_(self.c_loss)
            cursor_add(self.block, self.EPOCH, 1)
            cursor_add(self.block, self.BASE, self.m)

    @torch.no_grad()
    def run(self, state, action, old_prob, target, seed: int):
        """Copy the batch in, reset the cursors, upload the corrections of all steps, replay once per epoch."""
        learner = self.learner
        self.state.copy_(state)
        self.action.copy_(action)
        self.a_prob.copy_(old_prob)
        self.ret.copy_(target)
        seed = int(seed) & (2 ** 64 - 1)
        cursor_set(self.block, [0, 0, seed & 0xFFFFFFFF, seed >> 32])
        steps = self.epochs * self.m
        # fresh pinned tensors: torch's host allocator does not hand them out again before the copies that read them have run
        self.a_table.copy_(learner.actor_optimizer.correction_table(steps), non_blocking=True)
        self.c_table.copy_(learner.critic_optimizer.correction_table(steps), non_blocking=True)
        self.a_sum.zero_()
        self.c_sum.zero_()
        for _ in range(self.epochs):
            self.graph.replay()
        learner.actor_optimizer.advance(steps)
        learner.critic_optimizer.advance(steps)
        learner.training_step += steps
        return self.a_sum / max(steps, 1), self.c_sum / max(steps, 1), steps


def ppo_update(learner, batch, seed: int):
    """``PPOLearner.update`` with ``graph=True``."""
    if learner.before_clip is not None:
        raise ValueError("graph=True: a before_clip hook is host code between the launches; unset it or construct with graph=False")
    states = batch["state"]
    T, A, F = int(states.shape[0]) - 1, int(states.shape[1]), int(states.shape[-1])
    n = T * A
    m = (n + learner.batch_size - 1) // learner.batch_size
    if m > learner.graph_max_minibatches:
        raise ValueError("graph=True: %d minibatches per epoch, graph_max_minibatches is %d (it bounds the graph's node count and capture time)"
                         % (m, learner.graph_max_minibatches))
    if not learner.uses_kernels(min(learner.batch_size, max(n, 1))):
        raise ValueError("graph=True: the kernels do not take these networks")
    if n == 0:
        return None
    key = (T, A, F, learner.ppo_update_time, learner.batch_size)
    g = learner._graphs.get(key)
    if g is not None and g.signature != _signature((learner.actor, learner.critic)):      # a parameter or a gradient moved: every graph is stale
        learner._graphs.clear()
        g = None
    if g is None:
        g = learner._capture(key[:3])
    return g.run(states[:T].reshape(n, F), batch["action"].reshape(-1), batch["a_prob"].reshape(-1), batch["return"].reshape(-1), seed)


class DQNUpdateGraph:
    """One ``DQNLearner.update`` as one graph: sample -> TD target -> loss, backward and clamp -> Adam [and the blend]."""

    LEN, STEP, KEY = 0, 2, 4      # the cursor block: len (int64 = two words), step, -, key lo, key hi

    def __init__(self, learner):
        self.learner = learner
        self.dev = dev = learner.buffer.device
        self.bs = learner.batch_size
        self.block = torch.zeros(8, dtype=torch.int32, device=dev)
        self.table = torch.ones(2, dtype=torch.float32, device=dev)
        self.index = torch.zeros(self.bs, dtype=torch.int64, device=dev)
        self.y = torch.zeros(self.bs, dtype=torch.float32, device=dev)
        self.next_q = torch.zeros(self.bs, dtype=torch.float32, device=dev)
        self.next_action = torch.zeros(self.bs, dtype=torch.uint8, device=dev)
        self.loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.p_desc, self.t_desc = L.mlp_desc(L.fc_layers(learner.policy_net)), L.mlp_desc(L.fc_layers(learner.target_net))
        sizes, self.target_launch, self.grad_launch = learner._kernels()      # the learner's own calls (wide or narrow), on static buffers
        floats, nbytes = sizes(self.p_desc, self.bs)
        self.workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)      # the graph's own
        self.flat = _flat_grad(learner.policy_net, floats)
        opt = learner.optimizer
        held = list(learner.policy_net.parameters()) + list(learner.target_net.parameters()) + [opt._exp_avg, opt._exp_avg_sq]
        cursor_set(self.block, [1, 0, 0, 0])      # the warm-up pass reads row 0 of the (allocated, possibly empty) buffer
        self.graph = _capture(self._record, held, dev)
        self.signature = _signature((learner.policy_net, learner.target_net))

    def _record(self) -> None:
        learner, dev, buf = self.learner, self.dev, self.learner.buffer
        st = L.stream(dev)
        with torch.cuda.device(dev):
            sample(self.bs, self.block[self.LEN:self.LEN + 2].view(torch.int64), 0, 0, dev, out=self.index, cursor=self.block[self.STEP:],
                   key=self.block[self.KEY:])
            self.target_launch(self.t_desc, self.p_desc if learner.double else None, buf.next_state, buf.num_state, buf.reward, self.index, self.bs,
                               self.y, self.next_q, self.next_action, st)
            self.grad_launch(self.p_desc, buf.state, buf.num_state, buf.action, self.y, self.index, self.bs, self.workspace, self.flat, self.loss,
                             None, st)
            if learner.soft_update:
                learner.optimizer.step(target=learner._fused_target, tau=learner.tau, corrections=self.table, slot=0)
            else:
                learner.optimizer.step(corrections=self.table, slot=0)

    @torch.no_grad()
    def run(self, seed: int) -> torch.Tensor:
        learner = self.learner
        seed = int(seed) & (2 ** 64 - 1)
        cursor_set(self.block, [len(learner.buffer), 0, learner.training_step, 0])
        cursor_set(self.block, [seed & 0xFFFFFFFF, seed >> 32], offset=self.KEY)
        self.table.copy_(learner.optimizer.correction_table(1), non_blocking=True)
        self.graph.replay()
        learner.optimizer.advance(1)
        learner.training_step += 1
        return self.loss.clone()


def dqn_update(learner, seed: int) -> Optional[torch.Tensor]:
    """``DQNLearner.update`` with ``graph=True``."""
    if learner.before_step is not None:
        raise ValueError("graph=True: a before_step hook is host code between the launches; unset it or construct with graph=False")
    if len(learner.buffer) < learner.batch_size:
        return None
    if not learner.uses_kernels(learner.batch_size):
        raise ValueError("graph=True: the kernels do not take these networks")
    g = learner._graph
    if g is not None and (g.signature != _signature((learner.policy_net, learner.target_net)) or g.bs != learner.batch_size):
        g = None
    if g is None:
        g = learner._capture()
    return g.run(seed)
