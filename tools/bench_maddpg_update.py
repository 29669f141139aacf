#!/usr/bin/env python3
"""One update of MADDPG: mdr_amd.maddpg's kernels against torch autograd of the reference's expressions (agents/ddpg.py:305-339) on the
same replay buffer, same GPU, same session.  The parent of this feature has no MADDPG update: autograd - the learner's `torch` backend -
is what a user runs without it, and the baseline.  HIP events after warm-up, the two backends alternating; the median of `--repeats`
windows and their spread; one JSON line per (size, optimiser, what).

    python tools/bench_maddpg_update.py [--rows 64,256,4096] [--repeats 7] [--warmup 3] [--out FILE]

Three measurements per size and optimiser (torch.optim.Adam, mdr_amd.optim.FusedAdam):
  "critic step"   one agent's ``critic_backward`` (TD target through both target nets, mse loss, backward) + clip + Adam
  "actor step"    one agent's ``actor_backward`` (sample, critic forward and backward to two input columns, the actor's backward) + clip + Adam
  "update"        a whole ``MADDPGLearner.update``: the N agents in order, then the target blend
The reference's shape: N = 20 agents, F = 51, hidden 256-256, J = 1060 joint inputs; the buffer holds 8192 env-steps.

    python tools/bench_maddpg_update.py --graph-leg [--rows 64,256] [--repeats 7] [--iters 50] [--out FILE]

The graph leg: a whole update with ``backend="hip"`` and ``FusedAdam`` in three forms - "torch" (``sampler="torch"``: N ``randperm`` and one
``exponential_`` on the host side of every update, the code before the device-side draws), "philox" (``sampler="philox"``: one
mdr_maddpg_draws launch, the rest eager) and "graph" (``graph=True``: the update replayed from one captured graph) - with shared and with
per-agent networks.  Windows of ``--iters`` updates, the three forms alternating, ``--repeats`` windows each (7 x 50 = 350 updates per
form); per update the median window, the fastest and the slowest.  After the last window "philox" and "graph" have made the same
updates from the same nets: ``graph_bits_equal_philox`` says whether every parameter is bit-equal.
Per-kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_maddpg_update.py --only hip` in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from mdr_amd import maddpg  # noqa: E402
from mdr_amd.optim import FusedAdam  # noqa: E402

DEV = "cuda:0"
N, F_OBS, HIDDEN, CAPACITY = 20, 51, 256, 8192


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def learner_for(backend, B, optimizer, steps):
    torch.manual_seed(0)
    actor = maddpg.DDPGNetworkMLP(F_OBS, 2, HIDDEN).to(DEV)
    critic = maddpg.DDPGNetworkMLP(N * (F_OBS + 2), 1, HIDDEN).to(DEV)
    lrn = maddpg.MADDPGLearner(actor, critic, N, 1e-3, 3e-3, batch_size=B, buffer_capacity=CAPACITY, backend=backend, optimizer=optimizer)
    lrn.buffer.push(*steps)
    return lrn


def graph_leg(args, steps, emit):
    forms = (("torch", dict(sampler="torch")), ("philox", dict(sampler="philox")), ("graph", dict(graph=True)))
    for B in (int(x) for x in args.rows.split(",")):
        for shared in (True, False):
            lrn = {}
            for name, kw in forms:
                torch.manual_seed(0)
                n = 1 if shared else N
                actors = [maddpg.DDPGNetworkMLP(F_OBS, 2, HIDDEN).to(DEV) for _ in range(n)]
                critics = [maddpg.DDPGNetworkMLP(N * (F_OBS + 2), 1, HIDDEN).to(DEV) for _ in range(n)]
                lrn[name] = maddpg.MADDPGLearner(actors[0] if shared else actors, critics[0] if shared else critics, N, 1e-3, 3e-3, batch_size=B,
                                                 buffer_capacity=CAPACITY, backend="hip", optimizer=FusedAdam, shared=shared, **kw)
                lrn[name].buffer.push(*steps)
            t = {name: [] for name in lrn}
            for _ in range(args.warmup):
                for l in lrn.values():
                    l.update(seed=1)
            torch.cuda.synchronize()
            for _ in range(args.repeats):      # alternating windows
                for name, l in lrn.items():
                    t[name].append(window(lambda: l.update(seed=1), args.iters))
            equal = all(torch.equal(p, q) for a, b in zip(lrn["philox"].actors + lrn["philox"].critics, lrn["graph"].actors + lrn["graph"].critics)
                        for p, q in zip(a.parameters(), b.parameters()))
            rec = dict(what="update, three forms", rows=B, agents=N, shared=shared, iters_per_window=args.iters, repeats=args.repeats,
                       updates_per_form=args.iters * args.repeats, graph_bits_equal_philox=equal, graph_captures=lrn["graph"].graph_captures)
            for name, v in t.items():
                rec[name + "_us_median"] = round(statistics.median(v), 1)
                rec[name + "_us_min"], rec[name + "_us_max"] = round(min(v), 1), round(max(v), 1)
            for name in ("philox", "graph"):
                rec["torch_over_" + name] = round(statistics.median(t["torch"]) / statistics.median(t[name]), 3)
            emit(**rec)
            del lrn
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,256,4096")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--graph-leg", action="store_true", help="the three forms of the update (module docstring) instead of the backends' table")
    ap.add_argument("--iters", type=int, default=50, help="updates per window of the graph leg")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_maddpg_update.py needs a GPU"
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    gen = torch.Generator(device=DEV).manual_seed(1)
    steps = (torch.rand((CAPACITY, N, F_OBS), device=DEV, generator=gen) * 2 - 1, torch.randint(0, 2, (CAPACITY, N), device=DEV, generator=gen),
             torch.randn((CAPACITY, N), device=DEV, generator=gen), torch.rand((CAPACITY, N, F_OBS), device=DEV, generator=gen) * 2 - 1)
    backends = [b for b in ("hip", "torch") if args.only in (None, b)]
    rows = [int(x) for x in args.rows.split(",")]
    if args.graph_leg:
        graph_leg(args, steps, emit)
        rows = []
    for B in rows:
        for opt_name, opt in (("Adam", torch.optim.Adam), ("FusedAdam", FusedAdam)):
            lrn = {b: learner_for(b, B, opt, steps) for b in backends}
            index, noise_t, noise_a = next(iter(lrn.values())).draws(0)
            diff = None
            if len(backends) == 2:      # the two backends agree before anything is timed
                grads = {}
                for b in backends:
                    lrn[b].critic_backward(3, index[3], noise_t[3])
                    lrn[b].actor_backward(3, index[3], noise_a[3])
                    grads[b] = torch.cat([p.grad.reshape(-1) for net in (lrn[b].critic, lrn[b].actor) for p in net.parameters()]).clone()
                diff = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())

            def critic_step(l):
                l.critic_backward(3, index[3], noise_t[3])
                l._step(l.critic_optimizer, l.critic, None)

            def actor_step(l):
                l.actor_backward(3, index[3], noise_a[3])
                l._step(l.actor_optimizer, l.actor, None)

            whats = (("critic step", {b: (lambda l=lrn[b]: critic_step(l)) for b in backends}, max(3, min(200, 20000 // B + 3))),
                     ("actor step", {b: (lambda l=lrn[b]: actor_step(l)) for b in backends}, max(3, min(200, 20000 // B + 3))),
                     ("update", {b: lrn[b].update for b in backends}, max(2, min(10, 2000 // B + 2))))
            for what, fns, iters in whats:
                t = {b: [] for b in backends}
                for _ in range(args.warmup):
                    for b in backends:
                        fns[b]()
                torch.cuda.synchronize()
                for _ in range(args.repeats):      # alternating windows
                    for b in backends:
                        t[b].append(window(fns[b], iters))
                rec = dict(what=what, optimizer=opt_name, rows=B, agents=N, iters_per_window=iters, repeats=args.repeats,
                           max_rel_diff_of_gradients=diff)
                for b, v in t.items():
                    rec[b + "_us_median"] = round(statistics.median(v), 2)
                    rec[b + "_us_min"], rec[b + "_us_max"] = round(min(v), 2), round(max(v), 2)
                if len(backends) == 2:
                    rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
                emit(**rec)
            del lrn
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
