#!/usr/bin/env python3
"""The optimiser tail of an update - clip_grad_norm_ + torch.optim.Adam.step() (+ DQN's target blend) - against
mdr_amd.optim.FusedAdam.step(...), and whole learner updates with either optimiser, same GPU, same session.  The method of
tools/bench_dqn_update.py: HIP events around windows of calls after warm-up, `--repeats` windows per variant, the variants alternating,
median (min-max); one JSON line per measurement.

    python tools/bench_optim_step.py [--repeats 7] [--warmup 3] [--only tail|updates|default] [--out profiles/optim_step_bench.jsonl]
                                     [--readme profiles/optim_step_README.md] [--ratios-log FILE] [--parent-jsonl FILE]
    python tools/bench_optim_step.py --resources profiles/optim_step_kernel_resources.txt      (no GPU: the compiler's report)

(a) "tail": the tail alone on fixed gradients, at the reference's networks - F = 51, H = 100-100 actor and critic, the J = 70 joint
    critic, the one-hop TarMAC actor (24 tensors, 4 without a gradient), 1020-input TarMAC critics of 64, 128 and 256 hidden units - as torch, as FusedAdam in
    the one-launch form and in the two-launch form (max_fused_floats forced); and DQN's tail (Adam + blend, no clip) on the Q-network.
(b) "updates": DQNLearner.update at 256 and 65,536 rows (DQN, DDQN); PPOLearner / MAPPOLearner / TarMACPPOLearner.update over 256
    steps x 20 agents, ten epochs, minibatches of 256; optimizer=torch.optim.Adam against FusedAdam, hip backend.
(c) "default": the torch.optim.Adam variant of the 256-row DQN update alone, for the comparison with the parent commit (run the same
    command in a checkout of the parent: its tools/bench_dqn_update.py measures the same call; `--parent-jsonl` quotes it).
`--readme` writes the tables and the form switch they support; FusedAdam's shipped default of max_fused_floats is set from them.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
F_OBS, LAYERS = 51, (100, 100)
ONE, TWO = 1 << 30, 1


def resources(path):
    """VGPRs, SGPRs, scratch, LDS and occupancy of the kernels of csrc/mdr_optim.hip, as hipcc reports them for gfx950."""
    from mdr_amd import build
    src = os.path.join(build.CSRC, "mdr_optim.hip")
    cmd = [build._hipcc(), *build.FLAGS, "-c", src, "-o", os.devnull, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, cwd=build.CSRC, check=True, stderr=subprocess.PIPE, text=True).stderr
    rows = [re.sub(r"^.*remark: ", "", l).replace(" [-Rpass-analysis=kernel-resource-usage]", "") for l in err.splitlines() if "remark:" in l]
    with open(path, "w") as f:
        f.write("hipcc %s -c mdr_optim.hip -Rpass-analysis=kernel-resource-usage\n\n" % " ".join(build.FLAGS) + "\n".join(rows) + "\n")
    print("\n".join(rows))


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


def mlp_shapes(J, out):
    return [(LAYERS[0], J), (LAYERS[0],), (LAYERS[1], LAYERS[0]), (LAYERS[1],), (out, LAYERS[1]), (out,)]


def tail_networks():
    import torch
    from mdr_amd.tarmac import TarMACActor, TarMACCritic
    actor = TarMACActor(F_OBS)
    dead = [i for i, (n, _) in enumerate(actor.named_parameters()) if "msg_state2state" in n]
    return [("actor F=51 H=100-100", mlp_shapes(F_OBS, 2), []), ("critic F=51 H=100-100", mlp_shapes(F_OBS, 1), []),
            ("joint critic J=70", mlp_shapes(70, 1), []),
            ("one-hop TarMAC actor (20 of 24 tensors live)", [tuple(p.shape) for p in actor.parameters()], dead),
            ("TarMAC critic 1020 x 64", [tuple(p.shape) for p in TarMACCritic(20, F_OBS, 64).parameters()], []),
            ("TarMAC critic 1020 x 128", [tuple(p.shape) for p in TarMACCritic(20, F_OBS, 128).parameters()], []),
            ("TarMAC critic 1020 x 256", [tuple(p.shape) for p in TarMACCritic(20, F_OBS, 256).parameters()], [])]


def bench_tail(args, emit):
    import torch
    from mdr_amd.optim import FusedAdam
    gen = torch.Generator(device=DEV).manual_seed(1)

    def make(shapes, dead, opt):
        ps = [torch.nn.Parameter(torch.randn(s, device=DEV, generator=gen) * 0.1) for s in shapes]
        for i, p in enumerate(ps):
            if i not in dead:
                p.grad = torch.randn(p.shape, device=DEV, generator=gen)
        return ps, opt(ps)

    for name, shapes, dead in tail_networks():
        total = sum(int(torch.Size(s).numel()) for s in shapes)
        pt, adam = make(shapes, dead, lambda ps: torch.optim.Adam(ps, 1e-3))
        p1, one = make(shapes, dead, lambda ps: FusedAdam(ps, 1e-3, max_fused_floats=ONE))
        p2, two = make(shapes, dead, lambda ps: FusedAdam(ps, 1e-3, max_fused_floats=TWO))

        def torch_tail():
            torch.nn.utils.clip_grad_norm_(pt, 0.5)
            adam.step()

        rec = dict(what="tail: clip + Adam", network=name, floats=total, tensors=len(shapes), iters_per_window=200, repeats=args.repeats)
        rec.update(alternate({"torch": torch_tail, "fused_one_launch": lambda: one.step(max_grad_norm=0.5),
                              "fused_two_launches": lambda: two.step(max_grad_norm=0.5)}, 200, args.warmup, args.repeats))
        emit(**rec)
    # DQN's tail: no clip (the clamp is in the gradient's reduction), Adam and the blend
    shapes = mlp_shapes(F_OBS, 2)
    pt, adam = make(shapes, [], lambda ps: torch.optim.Adam(ps, 1e-3))
    pf, fused = make(shapes, [], lambda ps: FusedAdam(ps, 1e-3))
    tt, tf = [torch.zeros_like(p) for p in pt], [torch.zeros_like(p) for p in pf]

    def torch_tail():
        adam.step()
        with torch.no_grad():
            torch._foreach_mul_(tt, 0.99)
            torch._foreach_add_(tt, pt, alpha=0.01)

    rec = dict(what="tail: Adam + blend (DQN)", network="Q-network F=51 H=100-100", floats=sum(p.numel() for p in pt), tensors=6, iters_per_window=200,
               repeats=args.repeats)
    rec.update(alternate({"torch": torch_tail, "fused": lambda: fused.step(target=tf, tau=0.01)}, 200, args.warmup, args.repeats))
    emit(**rec)


def dqn_learner(opt, B, double):
    import torch
    from mdr_amd import dqn
    torch.manual_seed(0)
    lrn = dqn.DQNLearner(dqn.QNetworkMLP(F_OBS, layers=LAYERS).to(DEV), 1e-3, buffer_capacity=524288, batch_size=B, double=double, backend="hip",
                         optimizer=opt)
    gen = torch.Generator(device=DEV).manual_seed(1)
    C = lrn.buffer.capacity
    lrn.buffer.push(torch.rand((C, F_OBS), device=DEV, generator=gen) * 2 - 1, torch.randint(0, 2, (C,), device=DEV, generator=gen),
                    torch.randn(C, device=DEV, generator=gen), torch.rand((C, F_OBS), device=DEV, generator=gen) * 2 - 1)
    return lrn


def bench_default(args, emit):
    import torch
    lrn = dqn_learner(torch.optim.Adam, 256, False)
    rec = dict(what="dqn update, default optimiser (torch.optim.Adam)", rows=256, iters_per_window=200, repeats=args.repeats)
    rec.update(alternate({"torch_adam": lrn.update}, 200, args.warmup, args.repeats))
    emit(**rec)


def bench_updates(args, emit):
    import torch
    from mdr_amd import mappo, ppo, tarmac_ppo
    from mdr_amd.optim import FusedAdam
    from mdr_amd.rollout import ActorMLP, CriticMLP
    from mdr_amd.tarmac import TarMACActor, TarMACCritic
    opts = {"torch_adam": torch.optim.Adam, "fused_adam": FusedAdam}
    for B in (256, 65536):
        iters = max(3, min(200, int(2e6 // B) + 3))
        for double in (False, True):
            lrn = {k: dqn_learner(o, B, double) for k, o in opts.items()}
            rec = dict(what="%s update" % ("ddqn" if double else "dqn"), rows=B, iters_per_window=iters, repeats=args.repeats)
            rec.update(alternate({k: l.update for k, l in lrn.items()}, iters, args.warmup, args.repeats))
            emit(**rec)
            del lrn
            torch.cuda.empty_cache()
    T, N = 256, 20
    gen = torch.Generator(device=DEV).manual_seed(2)
    batch = dict(state=torch.rand((T + 1, N, F_OBS), device=DEV, generator=gen) * 2 - 1, action=torch.randint(0, 2, (T, N), device=DEV, generator=gen),
                 a_prob=0.3 + 0.4 * torch.rand((T, N), device=DEV, generator=gen))
    batch["return"] = torch.randn((T, N), device=DEV, generator=gen)
    kw = dict(clip_param=0.2, max_grad_norm=0.5, ppo_update_time=10, batch_size=256, backend="hip")

    def nets(kind):
        torch.manual_seed(0)
        if kind == "tarmac":
            return TarMACActor(F_OBS).to(DEV), TarMACCritic(N, F_OBS).to(DEV)
        return ActorMLP(F_OBS, layers=LAYERS).to(DEV), CriticMLP(F_OBS + (N - 1 if kind == "mappo" else 0), layers=LAYERS).to(DEV)

    for kind, cls in (("ppo", ppo.PPOLearner), ("mappo", mappo.MAPPOLearner), ("tarmac", tarmac_ppo.TarMACPPOLearner)):
        lrn = {k: cls(*nets(kind), 1e-3, 3e-3, optimizer=o, **kw) for k, o in opts.items()}
        count = next(iter(lrn.values())).update(batch, seed=0)[2]
        rec = dict(what="%s.update" % cls.__name__, steps=T, agents=N, epochs=10, batch_size=256, minibatches=count, iters_per_window=1, repeats=args.repeats)
        rec.update(alternate({k: (lambda l=l: l.update(batch, seed=0)) for k, l in lrn.items()}, 1, args.warmup, args.repeats))
        emit(**rec)


def run_trace(args, emit):
    """200 256-row DQN updates with FusedAdam and nothing else: the target of `rocprofv3 --kernel-trace --stats -- python
    tools/bench_optim_step.py --only trace`, in a run of its own."""
    import torch
    from mdr_amd.optim import FusedAdam
    lrn = dqn_learner(FusedAdam, 256, False)
    for _ in range(203):
        lrn.update()
    torch.cuda.synchronize()


def cell(r, k):
    return "%.1f (%.1f-%.1f)" % (r[k + "_us_median"], r[k + "_us_min"], r[k + "_us_max"])


def kernel_share(path):
    """-> (rows of `rocprofv3 --kernel-trace --stats`' kernel_stats.csv as (short name, calls, average us, percent), the csv's name)."""
    import csv
    with open(path) as f:
        rows = list(csv.DictReader(f))
    short = [(r["Name"].replace("void ", "").replace("(anonymous namespace)::", "").rsplit("(", 1)[0][:60], int(r["Calls"]),
              float(r["AverageNs"]) / 1e3, float(r["Percentage"])) for r in rows]
    return [r for r in short if r[1] >= 100], os.path.basename(path)


def write_readme(path, recs, ratios, parent, stats=None):
    tails = [r for r in recs if r["what"] == "tail: clip + Adam"]
    out = ["# The optimiser tail in one launch: `FusedAdam` (csrc/mdr_optim.hip)", "",
           "Written by `tools/bench_optim_step.py` from `profiles/optim_step_bench.jsonl`: one MI355X, one session, HIP events around windows of",
           "calls after warm-up, %d windows per variant, the variants alternating; every cell is the median (min-max) in microseconds." % (recs[0]["repeats"] if recs else 0),
           "Nothing here was fixed in advance; where a fused variant is slower than torch the table says so.", ""]
    if tails:
        out += ["## (a) The tail alone: `clip_grad_norm_` + `Adam.step()` against `FusedAdam.step(max_grad_norm=0.5)`", "",
                "| network | floats | tensors | torch | fused, one launch | fused, two launches | torch / best fused |", "|---|---|---|---|---|---|---|"]
        for r in tails:
            best = min(r["fused_one_launch_us_median"], r["fused_two_launches_us_median"])
            out.append("| %s | %d | %d | %s | %s | %s | %.2f |" % (r["network"], r["floats"], r["tensors"], cell(r, "torch"), cell(r, "fused_one_launch"),
                                                                   cell(r, "fused_two_launches"), r["torch_us_median"] / best))
        wins = [r["floats"] for r in tails if r["fused_one_launch_us_median"] <= r["fused_two_launches_us_median"]]
        loses = [r["floats"] for r in tails if r["fused_one_launch_us_median"] > r["fused_two_launches_us_median"]]
        out += ["", "**The form switch.**  The one-launch form was the faster of the two at %s floats and the slower at %s floats."
                % (", ".join(map(str, sorted(wins))) or "no size", ", ".join(map(str, sorted(loses))) or "no size")]
        if wins and loses and max(wins) < min(loses):
            out += ["Only these two sizes bracket the crossover: it lies between %d and %d floats and was not located more closely.  The shipped"
                    % (max(wins), min(loses)), "default of `max_fused_floats` is the larger measured size at which the one-launch form still wins, %d"
                    % max(wins), "(`DEFAULT_MAX_FUSED_FLOATS` in csrc/mdr_optim.hip).  Up to there both forms cost the host's time for one call or two",
                    "(the GPU is idle in between at these sizes); above it the %d workgroups that each re-read every gradient show." % (min(loses) // 1024)]
        out.append("")
    for r in recs:
        if r["what"].startswith("tail: Adam + blend"):
            out += ["DQN's tail (`Adam.step()` + the two `_foreach` launches of the blend, no clip) on the %s: torch %s, `FusedAdam.step(target=, tau=)` %s:"
                    % (r["network"], cell(r, "torch"), cell(r, "fused")), "torch / fused = %.2f." % (r["torch_us_median"] / r["fused_us_median"]), ""]
    ups = [r for r in recs if "torch_adam_us_median" in r and "fused_adam_us_median" in r]
    if ups:
        out += ["## (b) Whole updates, hip backend: `optimizer=torch.optim.Adam` against `optimizer=FusedAdam`", "",
                "| update | size | torch.optim.Adam | FusedAdam | torch / fused |", "|---|---|---|---|---|"]
        for r in ups:
            size = "%d rows" % r["rows"] if "rows" in r else "%d steps x %d agents, %d minibatches" % (r["steps"], r["agents"], r["minibatches"])
            out.append("| %s | %s | %s | %s | %.2f |" % (r["what"], size, cell(r, "torch_adam"), cell(r, "fused_adam"), r["torch_adam_us_median"] / r["fused_adam_us_median"]))
        slower = [r["what"] + (" at %d rows" % r["rows"] if "rows" in r else "") for r in ups if r["fused_adam_us_median"] > r["torch_adam_us_median"]]
        out += ["", "Slower with FusedAdam than with torch.optim.Adam: %s." % (", ".join(slower) if slower else "no case measured"), ""]
    dflt = [r for r in recs if r["what"].startswith("dqn update, default")]
    out += ["## The default path", ""]
    if dflt and parent:
        r = dflt[0]
        out += ["The 256-row DQN update with the default `torch.optim.Adam` (`tools/bench_dqn_update.py`'s \"dqn update\", hip backend): this commit %s." % cell(r, "torch_adam")]
        for q in parent:
            where = "below" if r["torch_adam_us_median"] < q["us_min"] else ("above" if r["torch_adam_us_median"] > q["us_max"] else "inside")
            out += ["The parent commit in the same session (its own tool, a process of its own): %.1f (%.1f-%.1f); this commit's median lies %s that spread."
                    % (q["us_median"], q["us_min"], q["us_max"], where)]
        out += [""]
    elif dflt:
        out += ["The 256-row DQN update with the default `torch.optim.Adam` on this commit: %s.  The parent commit was not measured in this session."
                % cell(dflt[0], "torch_adam"), ""]
    else:
        out += ["Not measured.", ""]
    out += ["## Error against the fp64 step", "",
            "tests/optim_ref.py derives a per-element bound for `p`, `m`, `v`, `target` and `total_norm` from the kernel's operation count",
            "(u = 2^-24, no fitted constant); tests/test_gpu_optim.py holds every element of every case to it - and torch's own fp32 step too."]
    out += ["Worst observed |error| / bound over that file: %s." % ratios if ratios else "Worst observed |error| / bound: not recorded in this run.", "",
            "`p` stands near 1 where the earlier features stood near 0.2, and that is one rounding, not a missed term: a step moves a parameter by",
            "about lr = 1e-3 of itself, so E_p is u |p'| - the bound of the final subtraction's own rounding - plus a thousandth of it, and a",
            "half-ulp error on an element whose mantissa is just above a power of two reaches u |p'| by itself.  torch's own fp32 step reaches",
            "0.96 on the same inputs (`test_torch_adam_with_clip_grad_norm_sits_inside_the_bound`); the quantities whose bound is made of several",
            "terms (`m`, `v`, `target`) stand at 0.49-0.58, `total_norm` at 0.12.", ""]
    if stats:
        rows, name = kernel_share(stats)
        out += ["## GPU time of the 256-row DQN update with FusedAdam", "",
                "`rocprofv3 --kernel-trace --stats -- python tools/bench_optim_step.py --only trace` (203 updates, a run of its own; `profiles/%s`," % name,
                "kernels with at least 100 calls).  `profiles/dqn_update_kernel_stats.csv` is the same update with torch's Adam and blend: nine",
                "`multi_tensor_apply` launches of 2.6-3.9 us each where `k_adam_step` stands here.", "", "| kernel | calls | average us | % of GPU time |", "|---|---|---|---|"]
        out += ["| `%s` | %d | %.2f | %.1f |" % r for r in rows]
        out += [""]
    out += ["## Not measured", "",
            "- The crossover of the two forms more closely than the two sizes above, and in GPU time alone: the windows time back-to-back calls, and up",
            "  to the crossover they measure the host's time per call (25 us for 6 tensors, 46 us for 24), not the kernel's.",
            "- Learners on the torch backend with FusedAdam, more than one GPU, and any network of more than 332,308 parameters.",
            "- No sanitizer run was made of the new host code.", ""]
    with open(path, "w") as f:
        f.write("\n".join(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("tail", "updates", "default", "trace"), default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None)
    ap.add_argument("--from-jsonl", default=None, help="write the README from recorded lines instead of measuring")
    ap.add_argument("--ratios-log", default=None, help="the output of pytest -s tests/test_gpu_optim.py: its last line is quoted")
    ap.add_argument("--parent-jsonl", default=None, help="the parent commit's tools/bench_dqn_update.py --only hip --rows 256 output (several: comma-separated)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3's kernel_stats.csv of `--only trace`, quoted in the README")
    ap.add_argument("--resources", default=None)
    args = ap.parse_args()
    if args.resources:
        resources(args.resources)
        return
    recs = []
    if args.from_jsonl:
        with open(args.from_jsonl) as f:
            recs = [json.loads(l) for l in f if l.strip()]
    else:
        import torch
        assert torch.cuda.is_available(), "bench_optim_step.py needs a GPU"

        def emit(**rec):
            recs.append(rec)
            print(json.dumps(rec), flush=True)

        for name, fn in (("tail", bench_tail), ("updates", bench_updates), ("default", bench_default), ("trace", run_trace)):
            if args.only == name or (args.only is None and name != "trace"):
                fn(args, emit)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(json.dumps(r) for r in recs) + "\n")
    if args.readme:
        ratios = parent = None
        if args.ratios_log and os.path.isfile(args.ratios_log):
            with open(args.ratios_log) as f:
                found = re.findall(r"worst \|error\| / bound over this file: (.*)", f.read())
            ratios = found[-1].strip() if found else None
        for path in (args.parent_jsonl or "").split(","):
            if not os.path.isfile(path):
                continue
            with open(path) as f:
                for l in f:
                    if l.startswith("{") and json.loads(l).get("what") == "dqn update" and json.loads(l).get("rows") == 256:
                        q = json.loads(l)
                        parent = (parent or []) + [dict(us_median=q["hip_us_median"], us_min=q["hip_us_min"], us_max=q["hip_us_max"])]
        write_readme(args.readme, recs, ratios, parent, args.kernel_stats if args.kernel_stats and os.path.isfile(args.kernel_stats) else None)


if __name__ == "__main__":
    main()
