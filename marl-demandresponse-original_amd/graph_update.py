"""Device-side minibatch indices and the captured update of PPOLearner, MAPPOLearner, DQNLearner, MADDPGLearner, TarMACPPOLearner and
TarMACA2CLearner (csrc/mdr_minibatch.hip, include/mdr_policy.h: mdr_minibatch_permutation, mdr_minibatch_sample, mdr_maddpg_draws, mdr_update_cursor_set,
mdr_adam_step_table).

At the reference's sizes an update is host time: a PPO minibatch is six launches of 60-80 us of GPU work behind 190 us of Python,
ctypes and launch overhead (profiles/optim_step_README.md).  Three host-side things keep an update from being replayed as a graph -
the minibatch indices (``torch.randperm`` under a generator seeded per epoch), Adam's bias corrections (kernel arguments formed from
the host's step count) and host counters.  Here each has a device-side counterpart:

* ``permutation`` / ``sample`` / ``maddpg_draws``: the indices (MADDPG: every agent's distinct positions and all gumbel noise of an
  update, one launch) as a function of (seed, epoch or step, element) through Philox - ``sampler="philox"`` of the learners, eager
  launches, usable on its own;
* ``FusedAdam.step(corrections=, slot=, base_dev=)``: the bias corrections from a table in device memory;
* a block of int32 cursors (epoch, table base, the seed as the Philox key; DQN: the buffer's fill count and the step) that one-thread
  kernels set and advance.

``PPOUpdateGraph`` holds ONE epoch - the permutation, every minibatch's critic call, actor call and two table steps, the loss sums,
the cursor advance - as one ``torch.cuda.CUDAGraph`` captured on one side stream (a chain of nodes, no fork); an update copies the batch
into the graph's static input buffers, resets the cursors, uploads the corrections of all its steps and replays the graph
``ppo_update_time`` times.  ``DQNUpdateGraph`` and ``MADDPGUpdateGraph`` hold one update each, reading the replay buffer in place.
``TarMACPPOUpdateGraph`` and ``TarMACA2CUpdateGraph`` hold one epoch over env-steps in the same way; the Philox key of TarMAC-PPO's
communication defects and its step come from the cursor block too (mdr_tarmac_ppo_actor_grad_keyed).  Nothing is allocated inside a capture, and a capture leaves no
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


def maddpg_draws(nb_agents: int, batch: int, length, seed: int, step: int, device, out=None, cursor: Optional[torch.Tensor] = None,
                 key: Optional[torch.Tensor] = None):
    """Everything one MADDPG update draws, by (seed, step), in one launch (mdr_maddpg_draws) -> (index int64 [N, B]: B distinct
    positions of [0, length) per agent; noise_t float32 [N, B, N, 2] and noise_a float32 [N, B, 2]: Gumbel(0, 1) noise).  ``out``:
    the three tensors to write (contiguous, of these shapes).  ``length``: an int >= B or one device int64 read when the kernel runs;
    ``cursor`` / ``key`` as ``permutation``'s (the cursor is added to the low word of ``step``)."""
    dev = torch.device(device)
    N, B = int(nb_agents), int(batch)
    if N < 1 or B < 0:
        raise ValueError("maddpg_draws: nb_agents >= 1 and batch >= 0")
    shapes = ((N, B), (N, B, N, 2), (N, B, 2))
    dtypes = (torch.int64, torch.float32, torch.float32)
    if out is None:
        out = tuple(torch.empty(s, dtype=d, device=dev) for s, d in zip(shapes, dtypes))
    if len(out) != 3 or any(t.shape != s or t.dtype != d or t.device != dev or not t.is_contiguous() for t, s, d in zip(out, shapes, dtypes)):
        raise ValueError("maddpg_draws: out must be contiguous (int64 %s, float32 %s, float32 %s) on %s" % (shapes + (dev,)))
    _check_int32(cursor, dev, 1, "maddpg_draws: cursor")
    _check_int32(key, dev, 2, "maddpg_draws: key")
    len_dev, len_host = None, 0
    if isinstance(length, torch.Tensor):
        if length.dtype != torch.int64 or length.device != dev or length.numel() != 1:
            raise ValueError("maddpg_draws: a device length must be one int64 on %s" % dev)
        len_dev = C.c_void_p(length.data_ptr())
    else:
        len_host = int(length)
        if len_host < 1 or B > len_host:
            raise ValueError("maddpg_draws: %d distinct positions asked of %d" % (B, len_host))
    lib = nat.load()
    cur = C.c_void_p(cursor.data_ptr()) if cursor is not None else None
    ptrs = [C.c_void_p(t.data_ptr()) for t in out]
    with torch.cuda.device(dev):
        if key is not None:
            rc = lib.mdr_maddpg_draws_keyed(N, B, len_dev, len_host, C.c_void_p(key.data_ptr()), int(step) & (2 ** 64 - 1), cur, *ptrs, L.stream(dev))
        else:
            rc = lib.mdr_maddpg_draws(N, B, len_dev, len_host, int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1), cur, *ptrs, L.stream(dev))
    nat.check(lib, None, rc, "mdr_maddpg_draws")
    return tuple(out)


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


def _flat_grad(net, floats: int, params: Optional[Sequence[torch.Tensor]] = None, keep: bool = False) -> torch.Tensor:
    """The flat gradient of ``net`` with the ``p.grad`` of ``params`` - the tensors it covers, in its order; default: the six of an
    ``fc`` MLP - rebound to views of it: the captured optimiser step reads them there.  ``keep``: a gradient held in a tensor of its
    own is copied into its view first, so that ``p.grad`` keeps its value."""
    params = L.mlp_params(L.fc_layers(net)) if params is None else list(params)
    flat = L.flat_grad(net, floats, params[0].device)
    if keep:
        off = 0
        for p in params:
            view = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
            if p.grad is not None and p.grad.data_ptr() != view.data_ptr():
                view.copy_(p.grad)
    L.publish(params, flat, L.REBIND)
    return flat


def _signature(nets) -> list:
    """Where the parameters and gradients of ``nets`` are; an entry is an ``fc`` MLP or the list of tensors itself."""
    sig = []
    for net in nets:
        for p in (net if isinstance(net, (list, tuple)) else L.mlp_params(L.fc_layers(net))):
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


class MADDPGUpdateGraph:
    """One ``MADDPGLearner.update`` as one graph: the draws, then for every agent in order target -> critic loss and gradient ->
    critic step -> actor loss and gradient -> actor step, the target blends where the eager update puts them (shared: on each net's
    last step; unshared: critic a's on its one step, the N actor blends after the loop).  A chain of nodes on one stream."""

    LEN, STEP, KEY = 0, 2, 4      # the cursor block: len (int64 = two words), step, -, key lo, key hi

    def __init__(self, learner):
        self.learner = learner
        self.dev = dev = learner.buffer.device
        self.N, self.bs, self.shared = learner.nb_agents, learner.batch_size, learner.shared
        N, B = self.N, self.bs
        n = self.nets = 1 if self.shared else N
        self.block = torch.zeros(8, dtype=torch.int32, device=dev)
        self.index = torch.zeros((N, B), dtype=torch.int64, device=dev)
        self.noise_t = torch.zeros((N, B, N, 2), dtype=torch.float32, device=dev)
        self.noise_a = torch.zeros((N, B, 2), dtype=torch.float32, device=dev)
        self.y = torch.zeros(B, dtype=torch.float32, device=dev)
        self.next_q = torch.zeros(B, dtype=torch.float32, device=dev)
        self.next_action = torch.zeros((B, N), dtype=torch.uint8, device=dev)
        self.a_loss = torch.zeros(N, dtype=torch.float32, device=dev)      # slot a: written by agent a's gradient kernel
        self.c_loss = torch.zeros(N, dtype=torch.float32, device=dev)
        # shared: one table of N pairs per net (slot a = the net's a-th step of the update); unshared: one pair per optimiser (row a)
        self.a_table = torch.ones((N, 2), dtype=torch.float32, device=dev)
        self.c_table = torch.ones((N, 2), dtype=torch.float32, device=dev)
        actors, critics = learner.actors[:n], learner.critics[:n]
        tgt_actors, tgt_critics = learner.tgt_actors[:n], learner.tgt_critics[:n]
        self.a_descs = [L.mlp_desc(L.fc_layers(m)) for m in actors]
        self.c_descs = [L.mlp_desc(L.fc_layers(m)) for m in critics]
        self.tc_descs = [L.mlp_desc(L.fc_layers(m)) for m in tgt_critics]
        # one descriptor: mdr_maddpg_target; a host array of N: mdr_maddpg_target_agents
        self.ta_desc = L.mlp_desc(L.fc_layers(tgt_actors[0])) if self.shared else L.mlp_descs([L.fc_layers(m) for m in tgt_actors])
        sizes, self.target_launch, self.critic_launch, self.actor_launch = learner._kernels()      # the learner's own calls, on static buffers
        a_floats, c_floats, nbytes = sizes(self.a_descs[0], self.c_descs[0], N, B)
        self.workspace = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)      # the graph's own: the shared one may be reallocated
        self.a_flats = [_flat_grad(m, a_floats) for m in actors]
        self.c_flats = [_flat_grad(m, c_floats) for m in critics]
        held = [p for m in actors + critics + tgt_actors + tgt_critics for p in m.parameters()]
        for opt in learner.actor_optimizers[:n] + learner.critic_optimizers[:n]:
            held += [opt._exp_avg, opt._exp_avg_sq]
        cursor_set(self.block, [max(len(learner.buffer), 1), 0, 0, 0])      # the warm-up pass reads rows the buffer holds (row 0 of an empty one)
        self.graph = _capture(self._record, held, dev)
        self.signature = _signature(maddpg_nets(learner))

    def _record(self) -> None:
        learner, dev, buf = self.learner, self.dev, self.learner.buffer
        N, B = self.N, self.bs
        st = L.stream(dev)
        ld = N * buf.num_state      # the buffer's env-steps are contiguous
        norm, tau = learner.MAX_GRAD_NORM, learner.soft_tau
        with torch.cuda.device(dev):
            maddpg_draws(N, B, self.block[self.LEN:self.LEN + 2].view(torch.int64), 0, 0, dev, out=(self.index, self.noise_t, self.noise_a),
                         cursor=self.block[self.STEP:], key=self.block[self.KEY:])
            for a in range(N):
                k = 0 if self.shared else a
                critic, actor = learner.critics[a], learner.actors[a]
                c_opt, a_opt = learner.critic_optimizers[a], learner.actor_optimizers[a]
                # shared: slot a of the net's table, the blend on its last step; unshared: the optimiser's one pair, critic a's blend
                # on its one step, no actor blend here (every later agent reads tgt_actors[a] as the previous update left it)
                c_table, a_table, slot = (self.c_table, self.a_table, a) if self.shared else (self.c_table[a], self.a_table[a], 0)
                c_blend = a == N - 1 if self.shared else True
                a_blend = a == N - 1 if self.shared else False
                self.target_launch(self.ta_desc, self.tc_descs[k], buf.next_state, ld, buf.reward, self.index[a], B, N, a, self.noise_t[a], self.y,
                                   self.next_q, self.next_action, st)
                self.critic_launch(self.c_descs[k], buf.state, ld, buf.action, self.index[a], B, N, self.y, self.workspace, self.c_flats[k],
                                   self.c_loss[a:a + 1], None, st)
                if c_blend:
                    L.clip_and_step(c_opt, critic.parameters(), norm, target=L.mlp_params(L.fc_layers(learner.tgt_critics[a])), tau=tau,
                                    corrections=c_table, slot=slot)
                else:
                    L.clip_and_step(c_opt, critic.parameters(), norm, corrections=c_table, slot=slot)
                self.actor_launch(self.a_descs[k], self.c_descs[k], buf.state, ld, buf.action, self.index[a], B, N, a, self.noise_a[a], self.workspace,
                                  self.a_flats[k], self.a_loss[a:a + 1], None, None, st)
                if a_blend:
                    L.clip_and_step(a_opt, actor.parameters(), norm, target=L.mlp_params(L.fc_layers(learner.tgt_actors[a])), tau=tau,
                                    corrections=a_table, slot=slot)
                else:
                    L.clip_and_step(a_opt, actor.parameters(), norm, corrections=a_table, slot=slot)
            if not self.shared:
                for a in range(N):
                    L.blend(L.mlp_params(L.fc_layers(learner.tgt_actors[a])), L.mlp_params(L.fc_layers(learner.actors[a])), tau)

    def _corrections(self, optimizers) -> torch.Tensor:
        """The pairs of this update's steps, [N, 2] on the host: the N next steps of the one shared optimiser, or the next step of
        each of the N.  A fresh pinned tensor, as ``correction_table``'s."""
        if self.shared:
            return optimizers[0].correction_table(self.N).view(self.N, 2)
        host = torch.empty((self.N, 2), dtype=torch.float32, pin_memory=True)
        for a, opt in enumerate(optimizers):
            host[a].copy_(opt.correction_table(1))
        return host

    @torch.no_grad()
    def run(self, seed: int):
        learner = self.learner
        seed = int(seed) & (2 ** 64 - 1)
        fill = len(learner.buffer)
        cursor_set(self.block, [fill & 0xFFFFFFFF, fill >> 32, learner.training_step, 0])
        cursor_set(self.block, [seed & 0xFFFFFFFF, seed >> 32], offset=self.KEY)
        self.a_table.copy_(self._corrections(learner.actor_optimizers), non_blocking=True)
        self.c_table.copy_(self._corrections(learner.critic_optimizers), non_blocking=True)
        self.graph.replay()
        steps = self.N if self.shared else 1
        for opt in learner.actor_optimizers[:self.nets] + learner.critic_optimizers[:self.nets]:
            opt.advance(steps)
        learner.training_step += 1
        return self.a_loss.clone(), self.c_loss.clone()


def maddpg_nets(learner) -> list:
    """Every net an update of ``learner`` reads or writes (shared: one of each kind)."""
    n = 1 if learner.shared else learner.nb_agents
    return learner.actors[:n] + learner.critics[:n] + learner.tgt_actors[:n] + learner.tgt_critics[:n]


def maddpg_update(learner, seed: int):
    """``MADDPGLearner.update`` with ``graph=True``."""
    if learner.before_step is not None:
        raise ValueError("graph=True: a before_step hook is host code between the launches; unset it or construct with graph=False")
    if len(learner.buffer) < learner.batch_size:
        return None
    if not learner.uses_kernels(learner.batch_size):
        raise ValueError("graph=True: the kernels do not take these networks")
    g = learner._graph
    if g is not None and (g.signature != _signature(maddpg_nets(learner)) or g.bs != learner.batch_size):
        g = None
    if g is None:
        g = learner._capture()
    return g.run(seed)


def _minibatch_rows(n: int, bs: int) -> set:
    """The env-step counts of an epoch's minibatches: a full one and the tail."""
    m = (n + bs - 1) // bs
    return {min(bs, n), n - (m - 1) * bs}


class TarMACPPOUpdateGraph:
    """One epoch of ``TarMACPPOLearner.update`` over a batch of n = T x E env-steps of N agents and F features as one graph: the
    permutation, then per minibatch the critic's two launches (loss, advantage, gradient), the actor's chain
    (mdr_tarmac_ppo_actor_grad_keyed), the ``zero_()`` on the key bias, the actor's clip + step, the critic's clip + step and the loss
    sums - the eager order -, then the cursor advance.  A chain of nodes on one stream.

    The communication defects are keyed by (seed, training_step) in the eager update.  Here the seed is the key of the cursor block
    and the step is ``j`` by value for minibatch ``j`` plus the STEP cursor, which ``run`` sets to ``training_step`` and the graph
    advances by the minibatches of an epoch.  The cursor is one int32 added to the low word of the step: the replay reproduces the
    eager keys as long as ``training_step`` plus the update's steps stays below 2^32 (past it the eager update carries into the high
    word, the cursor wraps)."""

    EPOCH, BASE, KEY, STEP = 0, 1, 2, 4      # the cursor block: epoch, table base, key lo, key hi, the defects' step

    def __init__(self, learner, T: int, A: int, N: int, F: int):
        from . import tarmac_ppo as tp      # (tarmac_ppo imports this module)
        self.learner, self.tp = learner, tp
        actor, critic = learner.actor, learner.critic
        dev = next(actor.parameters()).device
        self.dev = dev
        self.n, self.N, self.F, self.bs, self.epochs = T * (A // N), N, F, learner.batch_size, learner.ppo_update_time
        self.m = (self.n + self.bs - 1) // self.bs
        n = self.n
        self.state = torch.zeros((n, N, F), dtype=torch.float32, device=dev)
        self.action = torch.zeros((n, N), dtype=torch.int64, device=dev)
        self.a_prob = torch.ones((n, N), dtype=torch.float32, device=dev)
        self.ret = torch.zeros((n, N), dtype=torch.float32, device=dev)
        self.perm = torch.zeros(n, dtype=torch.int64, device=dev)
        self.block = torch.zeros(8, dtype=torch.int32, device=dev)
        self.a_table = torch.ones(2 * self.epochs * self.m, dtype=torch.float32, device=dev)
        self.c_table = torch.ones(2 * self.epochs * self.m, dtype=torch.float32, device=dev)
        self.a_sum = torch.zeros((), dtype=torch.float32, device=dev)
        self.c_sum = torch.zeros((), dtype=torch.float32, device=dev)
        self.a_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.c_loss = torch.zeros((), dtype=torch.float32, device=dev)
        self.adv = torch.zeros((min(self.bs, n), N), dtype=torch.float32, device=dev)
        self.a_params, self.c_params = tp._params(actor), L.mlp_params(tp._critic_layers(critic))
        self.a_desc, self.c_desc = tp._desc(actor), L.mlp_desc(tp._critic_layers(critic))
        rows = _minibatch_rows(n, self.bs)
        a_floats, a_bytes = zip(*(tp._actor_sizes(self.a_desc, B, N) for B in rows))
        c_floats, c_bytes = zip(*(tp._critic_sizes(self.c_desc, B) for B in rows))
        self.workspace = torch.empty(max(16, *a_bytes, *c_bytes), dtype=torch.uint8, device=dev)      # the graph's own: the shared one may be reallocated
        self.a_flat = _flat_grad(actor, a_floats[0], self.a_params, keep=True)
        self.c_flat = _flat_grad(critic, c_floats[0], self.c_params, keep=True)
        a_opt, c_opt = learner.actor_optimizer, learner.critic_optimizer
        # the warm-up pass writes the flat gradients too: they are held, so that every ``.grad`` keeps its value over a capture
        held = (list(actor.parameters()) + list(critic.parameters()) + [a_opt._exp_avg, a_opt._exp_avg_sq, c_opt._exp_avg, c_opt._exp_avg_sq]
                + [self.a_flat, self.c_flat])
        self.graph = _capture(self._record, held, dev)
        self.signature = tarmac_ppo_signature(learner)

    def _record(self) -> None:
        """The launches of one epoch on the current stream, from the static buffers alone."""
        learner, dev, tp, N = self.learner, self.dev, self.tp, self.N
        st = L.stream(dev)
        base = self.block[self.BASE:self.BASE + 1]
        key, step_dev = self.block[self.KEY:self.KEY + 2], self.block[self.STEP:self.STEP + 1]
        ld_actor, ld_critic = self.F, N * self.F      # the static state buffer is contiguous
        with torch.cuda.device(dev):
            permutation(self.n, 0, 0, dev, out=self.perm, cursor=self.block[self.EPOCH:], key=key)
            for j in range(self.m):
                index = self.perm[j * self.bs:(j + 1) * self.bs]      # a view (the last one shorter): slicing launches nothing
                B = int(index.shape[0])
                tp._critic_launch(self.c_desc, self.state, ld_critic, self.ret, index, B, self.workspace, self.c_flat, self.c_loss, None, self.adv, st)
                tp._actor_launch(self.a_desc, self.state, ld_actor, self.action, self.a_prob, index, B, N, self.adv, self.workspace, self.a_flat,
                                 self.a_loss, None, st, learner.clip_param, step=j, key=key, step_dev=step_dev)
                tp._zero_key_bias(learner.actor, self.a_flat, self.a_params)
                # comm.msg_state2state has no gradient: the optimiser's segment table skips it, here as in the eager step
                L.clip_and_step(learner.actor_optimizer, learner.actor.parameters(), learner.max_grad_norm, corrections=self.a_table, slot=j,
                                base_dev=base)
                L.clip_and_step(learner.critic_optimizer, learner.critic.parameters(), learner.max_grad_norm, corrections=self.c_table, slot=j,
                                base_dev=base)
                self.a_sum.add_(self.a_loss)
                self.c_sum.add_(self.c_loss)
            cursor_add(self.block, self.EPOCH, 1)
            cursor_add(self.block, self.BASE, self.m)
            cursor_add(self.block, self.STEP, self.m)

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
        cursor_set(self.block, [learner.training_step], offset=self.STEP)
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


def tarmac_ppo_signature(learner) -> list:
    """Every parameter of both networks (``comm.msg_state2state``, which has no gradient, included) and where its gradient is."""
    return _signature((list(learner.actor.parameters()), list(learner.critic.parameters())))


def _epoch_checks(learner, n: int) -> None:
    m = (n + learner.batch_size - 1) // learner.batch_size
    if m > learner.graph_max_minibatches:
        raise ValueError("graph=True: %d minibatches per epoch, graph_max_minibatches is %d (it bounds the graph's node count and capture time)"
                         % (m, learner.graph_max_minibatches))


def tarmac_ppo_update(learner, batch, seed: int, nb_houses: Optional[int] = None):
    """``TarMACPPOLearner.update`` with ``graph=True``."""
    from . import tarmac_ppo as tp
    states = batch["state"]
    N = int(nb_houses) if nb_houses is not None else int(learner.critic.critic[-1].out_features)
    T, A, F = int(states.shape[0]) - 1, int(states.shape[1]), int(states.shape[-1])
    if N < 1 or A % N:
        raise ValueError("TarMACPPOLearner.update: %d agents per step are no whole number of envs of %d houses" % (A, N))
    n = T * (A // N)
    _epoch_checks(learner, n)
    if n == 0:
        return None
    why = tp._refusal(learner.actor, N) or tp._critic_refusal(learner.critic)
    if why:
        raise ValueError("graph=True: %s" % why)
    for B in _minibatch_rows(n, learner.batch_size):
        if not learner.uses_kernels(B) or not learner.critic_uses_kernels(B):
            raise ValueError("graph=True: a minibatch of %d env-steps does not take the actor and the critic kernels" % B)
    if N != int(learner.critic.critic[-1].out_features) or F != learner.actor.num_obs:
        raise ValueError("graph=True: the batch holds %d houses of %d features, the networks take %d of %d"
                         % (N, F, int(learner.critic.critic[-1].out_features), learner.actor.num_obs))
    key = (T, A, N, F, learner.ppo_update_time, learner.batch_size)
    g = learner._graphs.get(key)
    if g is not None and g.signature != tarmac_ppo_signature(learner):      # a parameter or a gradient moved: every graph is stale
        learner._graphs.clear()
        g = None
    if g is None:
        g = learner._capture(key[:2] + (F,), N)
    return g.run(states[:T].reshape(n, N, F), batch["action"].reshape(n, N), batch["a_prob"].reshape(n, N), batch["return"].reshape(n, N), seed)


class TarMACA2CUpdateGraph:
    """One epoch of ``TarMACA2CLearner.update`` over a batch of n = T x E env-steps of N agents as one graph: the permutation, then
    per minibatch ``mdr_tarmac_a2c_grad`` on the static buffers, ONE clip + step over all parameters (the ``base.comm.*`` tensors
    have no gradient and stay skipped) and the sum of the three losses.  Nothing is drawn besides the permutation."""

    EPOCH, BASE, KEY = 0, 1, 2      # the cursor block: epoch, table base, key lo, key hi

    def __init__(self, learner, T: int, A: int, N: int, F: int):
        from . import tarmac_a2c as ta      # (tarmac_a2c imports this module)
        self.learner, self.ta = learner, ta
        policy = learner.policy
        dev = policy.dist.linear.weight.device
        self.dev = dev
        self.n, self.N, self.F, self.C, self.bs, self.epochs = T * (A // N), N, F, policy.comm_size, learner.batch_size, learner.nb_updates
        self.m = (self.n + self.bs - 1) // self.bs
        n = self.n
        self.obs = torch.zeros((n, N, F), dtype=torch.float32, device=dev)
        self.comm = torch.zeros((n, N, self.C), dtype=torch.float32, device=dev)
        self.action = torch.zeros((n, N), dtype=torch.int64, device=dev)
        self.ret = torch.zeros((n, N), dtype=torch.float32, device=dev)
        self.perm = torch.zeros(n, dtype=torch.int64, device=dev)
        self.block = torch.zeros(4, dtype=torch.int32, device=dev)
        self.table = torch.ones(2 * self.epochs * self.m, dtype=torch.float32, device=dev)
        self.losses = torch.zeros(3, dtype=torch.float32, device=dev)
        self.sums = torch.zeros(3, dtype=torch.float32, device=dev)
        self.params = ta._reached(policy)
        self.desc = ta._desc(policy)
        floats, nbytes = zip(*(ta._grad_sizes(self.desc, B, N) for B in _minibatch_rows(n, self.bs)))
        self.workspace = torch.empty(max(16, *nbytes), dtype=torch.uint8, device=dev)      # the graph's own
        self.flat = _flat_grad(policy, floats[0], self.params, keep=True)
        opt = learner.optimizer
        held = list(policy.parameters()) + [opt._exp_avg, opt._exp_avg_sq, self.flat]      # the flat gradient: ``.grad`` keeps its value over a capture
        self.graph = _capture(self._record, held, dev)
        self.signature = _signature((list(policy.parameters()),))

    def _record(self) -> None:
        """The launches of one epoch on the current stream, from the static buffers alone."""
        learner, dev, ta = self.learner, self.dev, self.ta
        st = L.stream(dev)
        base = self.block[self.BASE:self.BASE + 1]
        with torch.cuda.device(dev):
            permutation(self.n, 0, 0, dev, out=self.perm, cursor=self.block[self.EPOCH:], key=self.block[self.KEY:])
            for j in range(self.m):
                index = self.perm[j * self.bs:(j + 1) * self.bs]
                B = int(index.shape[0])
                ta._grad_launch(self.desc, self.obs, self.F, self.comm, self.C, self.action, self.ret, index, B, self.N, self.workspace, self.flat,
                                self.losses, None, None, st, learner.value_loss_coef, learner.entropy_coef)
                L.clip_and_step(learner.optimizer, learner.policy.parameters(), learner.max_grad_norm, corrections=self.table, slot=j, base_dev=base)
                self.sums.add_(self.losses)
            cursor_add(self.block, self.EPOCH, 1)
            cursor_add(self.block, self.BASE, self.m)

    @torch.no_grad()
    def run(self, obs, comm, action, ret, seed: int):
        learner = self.learner
        self.obs.copy_(obs)
        self.comm.copy_(comm)
        self.action.copy_(action)
        self.ret.copy_(ret)
        seed = int(seed) & (2 ** 64 - 1)
        cursor_set(self.block, [0, 0, seed & 0xFFFFFFFF, seed >> 32])
        steps = self.epochs * self.m
        self.table.copy_(learner.optimizer.correction_table(steps), non_blocking=True)      # a fresh pinned tensor, as PPOUpdateGraph's
        self.sums.zero_()
        for _ in range(self.epochs):
            self.graph.replay()
        learner.optimizer.advance(steps)
        learner.training_step += steps
        out = self.sums / max(steps, 1)
        return out[0], out[1], out[2], steps


def tarmac_a2c_update(learner, batch, seed: int, nb_agents: Optional[int] = None):
    """``TarMACA2CLearner.update`` with ``graph=True``."""
    from . import tarmac_a2c as ta
    states, comms = batch["state"], batch["comm"]
    T, A, F = int(states.shape[0]) - 1, int(states.shape[1]), int(states.shape[-1])
    N = int(nb_agents) if nb_agents is not None else A // int(batch["value"].shape[1])
    if N < 1 or A % N:
        raise ValueError("TarMACA2CLearner.update: %d agents per step are no whole number of envs of %d agents" % (A, N))
    n = T * (A // N)
    _epoch_checks(learner, n)
    if n == 0:
        return None
    why = ta._refusal(learner.policy, N)
    if why:
        raise ValueError("graph=True: %s" % why)
    for B in _minibatch_rows(n, learner.batch_size):
        if not learner.uses_kernels(B, N):
            raise ValueError("graph=True: a minibatch of %d env-steps of %d agents does not take the kernels" % (B, N))
    if F != learner.policy.nb_obs or int(comms.shape[-1]) != learner.policy.comm_size:
        raise ValueError("graph=True: the batch holds %d features and %d comm columns, the policy takes %d and %d"
                         % (F, int(comms.shape[-1]), learner.policy.nb_obs, learner.policy.comm_size))
    key = (T, A, N, F, learner.nb_updates, learner.batch_size)
    g = learner._graphs.get(key)
    if g is not None and g.signature != _signature((list(learner.policy.parameters()),)):
        learner._graphs.clear()
        g = None
    if g is None:
        g = learner._capture(key[:2] + (F,), N)
    Cc = learner.policy.comm_size
    return g.run(states[:T].reshape(n, N, F), comms[:T].reshape(n, N, Cc), batch["action"].reshape(n, N), batch["return"].reshape(n, N), seed)
