#!/usr/bin/env python3
"""Whole learner updates replayed from a captured graph (``graph=True``, mdr_amd/graph_update.py) against the eager update, at the
sizes of profiles/optim_step_README.md (b): PPOLearner / MAPPOLearner.update over 256 steps x 20 agents (ten epochs, minibatches of
256: 200 minibatches), DQNLearner.update at 256 and 65,536 rows (DQN, DDQN); optimizer=FusedAdam, hip backend throughout.  The
method of tools/bench_optim_step.py: HIP events around windows of calls after warm-up, `--repeats` windows per variant, the variants
of one process alternating, median (min-max); one JSON line per measurement.

    python tools/bench_graph_update.py [--repeats 7] [--warmup 3] [--out profiles/graph_update.jsonl]
    python tools/bench_graph_update.py --tree PATH --label parent [--out FILE]     the eager update of another checkout (the parent
                                                                                   commit's, built), a process of its own
    python tools/bench_graph_update.py --only trace                                the target of rocprofv3 --kernel-trace --stats
    python tools/bench_graph_update.py --from-jsonl A,B --kernel-stats CSV --readme profiles/graph_update_README.md

Columns: "eager" is the update as the default path runs it (sampler="torch"); "philox" the eager update on the device-side indices;
"graph" the replayed one.  With --tree only "eager" exists (the other checkout need not know the new arguments).
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
F_OBS, LAYERS = 51, (100, 100)
T, N = 256, 20


def window(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def alternate(fns, iters, warmup, repeats):
    import torch
    t = {k: [] for k in fns}
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for k, fn in fns.items():
            t[k].append(window(fn, iters))
    out = {}
    for k, v in t.items():
        out[k + "_us_median"], out[k + "_us_min"], out[k + "_us_max"] = round(statistics.median(v), 2), round(min(v), 2), round(max(v), 2)
    return out


def variants(new):
    return {"eager": {}, "philox": dict(sampler="philox"), "graph": dict(graph=True)} if new else {"eager": {}}


def dqn_learner(B, double, **kw):
    import torch
    from mdr_amd import dqn
    from mdr_amd.optim import FusedAdam
    torch.manual_seed(0)
    lrn = dqn.DQNLearner(dqn.QNetworkMLP(F_OBS, layers=LAYERS).to(DEV), 1e-3, buffer_capacity=524288, batch_size=B, double=double, backend="hip",
                         optimizer=FusedAdam, **kw)
    gen = torch.Generator(device=DEV).manual_seed(1)
    C = lrn.buffer.capacity
    lrn.buffer.push(torch.rand((C, F_OBS), device=DEV, generator=gen) * 2 - 1, torch.randint(0, 2, (C,), device=DEV, generator=gen),
                    torch.randn(C, device=DEV, generator=gen), torch.rand((C, F_OBS), device=DEV, generator=gen) * 2 - 1)
    return lrn


def ppo_batch():
    import torch
    gen = torch.Generator(device=DEV).manual_seed(2)
    batch = dict(state=torch.rand((T + 1, N, F_OBS), device=DEV, generator=gen) * 2 - 1, action=torch.randint(0, 2, (T, N), device=DEV, generator=gen),
                 a_prob=0.3 + 0.4 * torch.rand((T, N), device=DEV, generator=gen))
    batch["return"] = torch.randn((T, N), device=DEV, generator=gen)
    return batch


def ppo_learner(kind, **kw):
    import torch
    from mdr_amd import mappo, ppo
    from mdr_amd.optim import FusedAdam
    from mdr_amd.rollout import ActorMLP, CriticMLP
    torch.manual_seed(0)
    cls = mappo.MAPPOLearner if kind == "mappo" else ppo.PPOLearner
    return cls(ActorMLP(F_OBS, layers=LAYERS).to(DEV), CriticMLP(F_OBS + (N - 1 if kind == "mappo" else 0), layers=LAYERS).to(DEV), 1e-3, 3e-3,
               clip_param=0.2, max_grad_norm=0.5, ppo_update_time=10, batch_size=256, backend="hip", optimizer=FusedAdam, **kw)


def timed_capture(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 2)      # ms


def bench(args, emit, new):
    import torch
    batch = ppo_batch()
    for kind in ("ppo", "mappo"):
        lrn = {k: ppo_learner(kind, **kw) for k, kw in variants(new).items()}
        rec = dict(what="%s.update" % type(lrn["eager"]).__name__, label=args.label, steps=T, agents=N, epochs=10, batch_size=256, iters_per_window=1,
                   repeats=args.repeats)
        if new:
            rec["capture_ms"] = timed_capture(lambda: lrn["graph"]._capture((T, N, F_OBS)))
        rec["minibatches"] = lrn["eager"].update(batch, seed=0)[2]
        rec.update(alternate({k: (lambda l=l: l.update(batch, seed=0)) for k, l in lrn.items()}, 1, args.warmup, args.repeats))
        emit(**rec)
        del lrn
    for B in (256, 65536):
        iters = max(3, min(200, int(2e6 // B) + 3))
        for double in (False, True):
            lrn = {k: dqn_learner(B, double, **kw) for k, kw in variants(new).items()}
            rec = dict(what="%s update" % ("ddqn" if double else "dqn"), label=args.label, rows=B, iters_per_window=iters, repeats=args.repeats)
            if new:
                rec["capture_ms"] = timed_capture(lrn["graph"]._capture)
            rec.update(alternate({k: l.update for k, l in lrn.items()}, iters, args.warmup, args.repeats))
            emit(**rec)
            del lrn
            torch.cuda.empty_cache()


def run_trace(args, emit):
    """Three graphed PPO updates (600 minibatches after the capture's warm-up pass) and 203 graphed 256-row DQN updates, nothing else."""
    import torch
    batch = ppo_batch()
    lrn = ppo_learner("ppo", graph=True)
    for _ in range(3):
        lrn.update(batch, seed=0)
    dq = dqn_learner(256, False, graph=True)
    for _ in range(203):
        dq.update()
    torch.cuda.synchronize()


def cell(r, k):
    return "%.1f (%.1f-%.1f)" % (r[k + "_us_median"], r[k + "_us_min"], r[k + "_us_max"]) if k + "_us_median" in r else "not measured"


def size_of(r):
    return "%d rows" % r["rows"] if "rows" in r else "%d steps x %d agents, %d minibatches" % (r["steps"], r["agents"], r["minibatches"])


def kernel_rows(path):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    return [(r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").rsplit("(", 1)[0][:70], int(r["Calls"]), float(r["AverageNs"]) / 1e3,
             float(r["TotalDurationNs"]) / 1e3) for r in rows]


def write_readme(path, recs, stats, notes):
    mine = [r for r in recs if r.get("label") != "parent"]
    parent = {}
    for r in recs:      # several parent runs of one size: the median of the medians, the widest spread
        if r.get("label") == "parent":
            parent.setdefault((r["what"], r.get("rows")), []).append(r)
    parent = {k: dict(eager_us_median=statistics.median(r["eager_us_median"] for r in v), eager_us_min=min(r["eager_us_min"] for r in v),
                      eager_us_max=max(r["eager_us_max"] for r in v)) for k, v in parent.items()}
    out = ["# Updates replayed from a captured graph: `graph=True` (mdr_amd/graph_update.py, csrc/mdr_minibatch.hip)", "",
           "Written by `tools/bench_graph_update.py` from `profiles/graph_update.jsonl`: one MI355X, one session, HIP events around windows of calls",
           "after warm-up, %d windows per variant, the variants of one process alternating; every cell is the median (min-max) in microseconds"
           % (mine[0]["repeats"] if mine else 0),
           "per update.  `optimizer=FusedAdam`, hip backend.  The parent commit's column is its own tree, built, in a process of its own in the same",
           "session.  No ratio was fixed in advance.", "",
           "| update | size | parent, eager | this commit, eager (`sampler=\"torch\"`) | eager, `sampler=\"philox\"` | `graph=True` | eager / graph | capture, ms |",
           "|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for r in mine:
        p = parent.get((r["what"], r.get("rows")))
        ratio = "%.2f" % (r["eager_us_median"] / r["graph_us_median"]) if "graph_us_median" in r else "-"
        out.append("| %s | %s | %s | %s | %s | %s | %s | %s |" % (r["what"], size_of(r), cell(p, "eager") if p else "not measured", cell(r, "eager"), cell(r, "philox"),
                                                                cell(r, "graph"), ratio, r.get("capture_ms", "-")))
        name = "%s at %s" % (r["what"], size_of(r))
        if "graph_us_median" in r:
            pays = r["graph_us_max"] < r["eager_us_min"]
            verdicts.append("- %s: the graphed range lies %s the eager range%s." % (name, "wholly below" if pays else "NOT wholly below",
                                                                                    "" if pays else " - the feature does not pay here"))
        if p:
            inside = p["eager_us_min"] <= r["eager_us_median"] <= p["eager_us_max"]
            verdicts.append("  The default path: this commit's eager median %.1f lies %s the parent's spread %.1f-%.1f."
                            % (r["eager_us_median"], "inside" if inside else ("below" if r["eager_us_median"] < p["eager_us_min"] else "ABOVE"),
                               p["eager_us_min"], p["eager_us_max"]))
    out += ["", "The feature counts as paying where the graphed range (min-max) lies wholly below the eager range at the same size:", ""] + verdicts + [""]
    if stats:
        rows = kernel_rows(stats)
        out += ["## The floor: the kernels' summed GPU time", "",
                "`rocprofv3 --kernel-trace --stats -- python tools/bench_graph_update.py --only trace` in a run of its own, no counters: three graphed",
                "PPO updates (600 minibatches, plus the 20 of the capture's warm-up pass) and 203 graphed 256-row DQN updates (plus one warm-up).", "",
                "| kernel | calls | average us | total us |", "|---|---|---|---|"]
        out += ["| `%s` | %d | %.2f | %.0f |" % r for r in rows if r[1] >= 3]
        out += [""]
    out += notes
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("updates", "trace"), default="updates")
    ap.add_argument("--tree", default=None, help="measure the eager update of the checkout at this path instead of this one")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None)
    ap.add_argument("--from-jsonl", default=None, help="write the README from recorded lines (several files: comma-separated) instead of measuring")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's kernel_stats.csv of `--only trace`")
    ap.add_argument("--notes", default=None, help="a markdown file appended to the README (what the tables cannot say)")
    args = ap.parse_args()
    recs = []
    if args.from_jsonl:
        for path in args.from_jsonl.split(","):
            with open(path) as f:
                recs += [json.loads(l) for l in f if l.startswith("{")]
    else:
        sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
        import torch
        assert torch.cuda.is_available(), "bench_graph_update.py needs a GPU"

        def emit(**rec):
            recs.append(rec)
            print(json.dumps(rec), flush=True)

        if args.only == "trace":
            run_trace(args, emit)
        else:
            bench(args, emit, new=args.tree is None)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(json.dumps(r) for r in recs) + "\n")
    if args.readme:
        notes = []
        if args.notes and os.path.isfile(args.notes):
            with open(args.notes) as f:
                notes = f.read().splitlines()
        write_readme(args.readme, recs, args.kernel_stats if args.kernel_stats and os.path.isfile(args.kernel_stats) else None, notes)


if __name__ == "__main__":
    main()
