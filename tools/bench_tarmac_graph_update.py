#!/usr/bin/env python3
"""TarMACPPOLearner / TarMACA2CLearner updates replayed from a captured graph (``graph=True``, mdr_amd/graph_update.py) against the
eager update, on the protocol of tools/bench_graph_update.py: HIP events around windows of calls after warm-up, `--repeats` windows per
variant, the variants of one process alternating, median (min-max); one JSON line per measurement.

Sizes: the reference's - TarMAC-PPO at 256 env-steps x 20 agents per minibatch with ppo_update_time = 10, TarMAC A2C at 128 x 20 with
10 updates, four minibatches per epoch each - and one where the GPU is expected to be busy anyway: 4096 env-steps x 20 agents per
minibatch (two minibatches per epoch).  hip backend (actor and critic), optimizer=FusedAdam throughout.

    python tools/bench_tarmac_graph_update.py [--repeats 7] [--warmup 2] [--out profiles/tarmac_graph_update.jsonl]
    python tools/bench_tarmac_graph_update.py --tree PATH --label parent [--out FILE]     the eager update of another checkout (the
                                                                                          parent commit's, built), a process of its own
    python tools/bench_tarmac_graph_update.py --from-jsonl A,B --readme profiles/tarmac_graph_update_README.md [--notes FILE]

Columns: "eager" is the update as the default path runs it (sampler="torch"); "philox" the eager update on the device-side indices;
"graph" the replayed one.  With --tree only "eager" exists (the other checkout need not know the new arguments).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N, F_OBS = 20, 22
# (learner, env-steps per minibatch, minibatches per epoch, epochs)
SIZES = (("tarmac_ppo", 256, 4, 10), ("tarmac_a2c", 128, 4, 10), ("tarmac_ppo", 4096, 2, 10), ("tarmac_a2c", 4096, 2, 10))


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
        out[k + "_us_windows"] = [round(x, 2) for x in v]
    return out


def variants(new):
    return {"eager": {}, "philox": dict(sampler="philox"), "graph": dict(graph=True)} if new else {"eager": {}}


def batch_of(kind, T, E, comm_size):
    import torch
    gen = torch.Generator(device=DEV).manual_seed(2)
    A = E * N
    batch = dict(state=torch.rand((T + 1, A, F_OBS), device=DEV, generator=gen) * 2 - 1, action=torch.randint(0, 2, (T, A), device=DEV, generator=gen),
                 a_prob=0.3 + 0.4 * torch.rand((T, A), device=DEV, generator=gen))
    batch["return"] = torch.randn((T, A), device=DEV, generator=gen)
    if kind == "tarmac_a2c":
        batch["comm"] = torch.randn((T + 1, A, comm_size), device=DEV, generator=gen)
        batch["value"] = torch.randn((T + 1, E), device=DEV, generator=gen)
    return batch


def learner_of(kind, batch_size, epochs, **kw):
    import torch
    from mdr_amd.optim import FusedAdam
    torch.manual_seed(0)
    if kind == "tarmac_ppo":
        from mdr_amd import tarmac_ppo
        from mdr_amd.tarmac import TarMACActor, TarMACCritic
        return tarmac_ppo.TarMACPPOLearner(TarMACActor(F_OBS).to(DEV), TarMACCritic(N, F_OBS).to(DEV), 1e-3, 3e-3, clip_param=0.2, max_grad_norm=0.5,
                                           ppo_update_time=epochs, batch_size=batch_size, backend="hip", critic_backend="hip", optimizer=FusedAdam, **kw)
    from mdr_amd import tarmac_a2c
    return tarmac_a2c.TarMACA2CLearner(tarmac_a2c.TarMACA2CPolicy(F_OBS).to(DEV), nb_updates=epochs, batch_size=batch_size, backend="hip",
                                       optimizer=FusedAdam, **kw)


def timed_capture(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return round((time.perf_counter() - t0) * 1e3, 2)      # ms


def bench(args, emit, new):
    import torch
    for kind, bs, m, epochs in SIZES:
        if args.only and args.only != kind:
            continue
        E = 8
        T = bs * m // E
        lrn = {k: learner_of(kind, bs, epochs, **kw) for k, kw in variants(new).items()}
        batch = batch_of(kind, T, E, 32)
        iters = 10 if bs <= 256 else 2      # updates per window: a window is some tenths of a second at either size
        rec = dict(what="%s.update" % type(lrn["eager"]).__name__, label=args.label, env_steps_per_minibatch=bs, agents=N, epochs=epochs,
                   iters_per_window=iters, repeats=args.repeats)
        if new:
            shape = (T, E * N, F_OBS)
            rec["capture_ms"] = timed_capture((lambda: lrn["graph"]._capture(shape)) if kind == "tarmac_ppo" else (lambda: lrn["graph"]._capture(shape, N)))
        rec["minibatches"] = lrn["eager"].update(batch, seed=0)[-1]
        rec.update(alternate({k: (lambda l=l: l.update(batch, seed=0)) for k, l in lrn.items()}, iters, args.warmup, args.repeats))
        emit(**rec)
        del lrn, batch
        torch.cuda.empty_cache()


def cell(r, k):
    return "%.0f (%.0f-%.0f)" % (r[k + "_us_median"], r[k + "_us_min"], r[k + "_us_max"]) if r and k + "_us_median" in r else "not measured"


def size_of(r):
    return "%d env-steps x %d agents per minibatch, %d minibatches" % (r["env_steps_per_minibatch"], r["agents"], r["minibatches"])


def write_readme(path, recs, notes):
    mine = [r for r in recs if r.get("label") != "parent"]
    parent = {}
    for r in recs:      # several parent runs of one size: the median of the medians, the widest spread
        if r.get("label") == "parent":
            parent.setdefault((r["what"], r["env_steps_per_minibatch"]), []).append(r)
    parent = {k: dict(eager_us_median=statistics.median(r["eager_us_median"] for r in v), eager_us_min=min(r["eager_us_min"] for r in v),
                      eager_us_max=max(r["eager_us_max"] for r in v)) for k, v in parent.items()}
    out = ["# TarMAC-PPO and TarMAC A2C updates replayed from a captured graph: `graph=True` (mdr_amd/graph_update.py)", "",
           "Written by `tools/bench_tarmac_graph_update.py` from `profiles/tarmac_graph_update.jsonl` (the raw windows are there): one MI355X, one",
           "session, HIP events around windows of 10 updates (2 at 4096 env-steps per minibatch) after warm-up, %d windows per variant, the variants of one process alternating; every"
           % (mine[0]["repeats"] if mine else 0),
           "cell is the median (min-max) in microseconds per update.  `optimizer=FusedAdam`, hip backend for actor, critic and policy, 20 agents of",
           "22 features, the default networks, `comm_defect_prob = 0`.  The parent commit's column is its own tree, built, in a process of its own in",
           "the same session.  No ratio was fixed in advance.", "",
           "| update | size | parent, eager | this commit, eager (`sampler=\"torch\"`) | eager, `sampler=\"philox\"` | `graph=True` | eager / graph | capture, ms |",
           "|---|---|---|---|---|---|---|---|"]
    verdicts = []
    for r in mine:
        p = parent.get((r["what"], r["env_steps_per_minibatch"]))
        ratio = "%.2f" % (r["eager_us_median"] / r["graph_us_median"]) if "graph_us_median" in r else "-"
        out.append("| %s | %s | %s | %s | %s | %s | %s | %s |" % (r["what"], size_of(r), cell(p, "eager"), cell(r, "eager"), cell(r, "philox"), cell(r, "graph"),
                                                                ratio, r.get("capture_ms", "-")))
        name = "%s at %s" % (r["what"], size_of(r))
        if "graph_us_median" in r:
            pays = r["graph_us_max"] < r["eager_us_min"]
            verdicts.append("- %s: the graphed range lies %s the eager range%s." % (name, "wholly below" if pays else "NOT wholly below",
                                                                                    "" if pays else " - the feature does not pay here"))
        if p:
            inside = p["eager_us_min"] <= r["eager_us_median"] <= p["eager_us_max"]
            verdicts.append("  The default path: this commit's eager median %.0f lies %s the parent's spread %.0f-%.0f."
                            % (r["eager_us_median"], "inside" if inside else ("below" if r["eager_us_median"] < p["eager_us_min"] else "ABOVE"),
                               p["eager_us_min"], p["eager_us_max"]))
    out += ["", "The feature counts as paying where the graphed range (min-max) lies wholly below the eager range at the same size; the default path",
            "counts as unchanged where this commit's eager median lies inside the parent's spread:", ""] + verdicts + [""]
    out += notes
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("tarmac_ppo", "tarmac_a2c"), default=None)
    ap.add_argument("--tree", default=None, help="measure the eager update of the checkout at this path instead of this one")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None)
    ap.add_argument("--from-jsonl", default=None, help="write the README from recorded lines (several files: comma-separated) instead of measuring")
    ap.add_argument("--notes", default=None, help="a markdown file appended to the README (what the table cannot say)")
    args = ap.parse_args()
    recs = []
    if args.from_jsonl:
        for path in args.from_jsonl.split(","):
            with open(path) as f:
                recs += [json.loads(l) for l in f if l.startswith("{")]
    else:
        sys.path.insert(0, os.path.abspath(args.tree) if args.tree else ROOT)
        import torch
        assert torch.cuda.is_available(), "bench_tarmac_graph_update.py needs a GPU"

        def emit(**rec):
            recs.append(rec)
            print(json.dumps(rec), flush=True)

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
        write_readme(args.readme, recs, notes)


if __name__ == "__main__":
    main()
