#!/usr/bin/env python3
"""One update of MADDPG with per-agent networks (``MADDPGLearner(shared=False)``) in its four forms, same replay buffer, same GPU, same
process: the method of tools/bench_maddpg_update.py - HIP events after ``--warmup`` updates, the forms alternating in windows of
``--iters`` updates, ``--repeats`` windows each; per update the median window, the fastest and the slowest; one JSON line per size.

    python tools/bench_maddpg_agents.py [--rows 64,256] [--repeats 7] [--iters 20] [--warmup 3] [--out FILE]

  "sequential"  ``backend="hip"``, ``FusedAdam``, ``sampler="philox"``, eager: the agents one after the other        } the parent's forms:
  "graph"       the same with ``graph=True``: the update replayed from one captured graph                            } the baseline
  "batched"     ``agent_steps="batched"``, eager: the agents side by side, about ten launches
  "torch"       ``backend="torch"`` with ``torch.optim.Adam``: autograd, what a user runs without the kernels

The reference's shape: N = 20 agents, F = 51, hidden 256-256, J = 1060 joint inputs; the buffer holds 8192 env-steps.  Before anything
is timed "sequential", "graph" and "batched" have made the warm-up updates from the same nets with the same seeds:
``batched_bits_equal_sequential`` is asserted, ``graph_bits_equal_sequential`` reported.  The yardstick of "batched" is "graph" in the
same run; a difference counts from three times the run-to-run spread (profiles/r11_README.md).
Per-kernel times come from ``rocprofv3 --kernel-trace --stats -- python tools/bench_maddpg_agents.py --only batched --rows 64`` in a
run of its own.
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
FORMS = (("sequential", dict(backend="hip", optimizer=FusedAdam, sampler="philox")),
         ("graph", dict(backend="hip", optimizer=FusedAdam, graph=True)),
         ("batched", dict(backend="hip", optimizer=FusedAdam, sampler="philox", agent_steps="batched")),
         ("torch", dict(backend="torch", optimizer=torch.optim.Adam, sampler="philox")))


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def learner_for(kw, B, steps):
    torch.manual_seed(0)      # every form starts from the same 2 N nets
    actors = [maddpg.DDPGNetworkMLP(F_OBS, 2, HIDDEN).to(DEV) for _ in range(N)]
    critics = [maddpg.DDPGNetworkMLP(N * (F_OBS + 2), 1, HIDDEN).to(DEV) for _ in range(N)]
    lrn = maddpg.MADDPGLearner(actors, critics, N, 1e-3, 3e-3, batch_size=B, buffer_capacity=CAPACITY, shared=False, **kw)
    lrn.buffer.push(*steps)
    return lrn


def same_bits(one, two):
    groups = lambda l: l.actors + l.critics + l.tgt_actors + l.tgt_critics      # noqa: E731
    return all(torch.equal(p, q) for a, b in zip(groups(one), groups(two)) for p, q in zip(a.parameters(), b.parameters()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="64,256")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20, help="updates per window")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None, help="comma-separated forms (default: all four)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_maddpg_agents.py needs a GPU"
    names = [n for n, _ in FORMS] if args.only is None else args.only.split(",")
    assert all(n in dict(FORMS) for n in names), names
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    gen = torch.Generator(device=DEV).manual_seed(1)
    steps = (torch.rand((CAPACITY, N, F_OBS), device=DEV, generator=gen) * 2 - 1, torch.randint(0, 2, (CAPACITY, N), device=DEV, generator=gen),
             torch.randn((CAPACITY, N), device=DEV, generator=gen), torch.rand((CAPACITY, N, F_OBS), device=DEV, generator=gen) * 2 - 1)
    for B in (int(x) for x in args.rows.split(",")):
        lrn = {n: learner_for(dict(FORMS)[n], B, steps) for n in names}
        for u in range(args.warmup):
            for l in lrn.values():
                l.update(seed=u)
        torch.cuda.synchronize()
        rec = dict(what="unshared update, four forms", rows=B, agents=N, iters_per_window=args.iters, repeats=args.repeats,
                   updates_per_form=args.iters * args.repeats)
        if "sequential" in lrn and "batched" in lrn:
            rec["batched_bits_equal_sequential"] = same_bits(lrn["sequential"], lrn["batched"])
            assert rec["batched_bits_equal_sequential"], "the batched update left other bits than the sequential one"
        if "sequential" in lrn and "graph" in lrn:
            rec["graph_bits_equal_sequential"] = same_bits(lrn["sequential"], lrn["graph"])
        t = {n: [] for n in lrn}
        for _ in range(args.repeats):      # alternating windows
            for n, l in lrn.items():
                t[n].append(window(lambda: l.update(seed=1), args.iters))
        for n, v in t.items():
            rec[n + "_us_median"] = round(statistics.median(v), 1)
            rec[n + "_us_min"], rec[n + "_us_max"] = round(min(v), 1), round(max(v), 1)
        for n in ("sequential", "graph", "torch"):
            if n in t and "batched" in t:
                rec[n + "_over_batched"] = round(statistics.median(t[n]) / statistics.median(t["batched"]), 3)
        emit(**rec)
        del lrn
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
