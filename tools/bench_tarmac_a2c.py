#!/usr/bin/env python3
"""TarMAC A2C: mdr_amd.tarmac_a2c's kernels against torch on the same module, same buffers, same GPU, same process.  HIP events
after warm-up, the two paths alternating; the median of `--repeats` windows, their minimum and maximum; one JSON line per record.

    python tools/bench_tarmac_a2c.py [--sizes 20x128,50x128,20x4096] [--envs 1,4096] [--repeats 7] [--warmup 3] [--out FILE] [--readme FILE]

Two kinds of record (F = 51, S = 128, C = 32, K = 16: the reference's sizes on the 51-feature observation):
  "loss backward"  one minibatch's losses + gradient: ``loss_backward`` (mdr_tarmac_a2c_grad, four launches) against
                   ``zero_grad()`` + ``dense_losses`` on ``forward_dense`` of the gathered minibatch + ``backward()`` - the comparator,
                   not the code under test; sizes are agents x env-steps per minibatch, the buffer holds twice the minibatch
  "update step"    the same + clip_grad_norm_ + Adam, as ``TarMACA2CLearner.step_minibatch`` runs it
  "act"            one act step over E envs of 20 agents: ``policy.act`` on the kernels (mdr_tarmac_a2c_forward, mdr_logits_sample,
                   mdr_tarmac_a2c_comm) against ``act(kernels=False)`` (eager ``forward_dense``, the same sampling kernel)
A record's ``wins`` says whether the kernels beat torch by more than the comparator's own run-to-run spread:
torch median - hip median > torch max - torch min.  ``backend="auto"`` and the default act path take their ranges from these records.
"""
import argparse
import copy
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from mdr_amd import tarmac_a2c as A  # noqa: E402

DEV = "cuda:0"
F_OBS, STATE, COMM, KEY = 51, 128, 32, 16
VC, EC, MAX_NORM, LR = 0.5, 0.01, 0.5, 7e-4


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def measure(fns, iters, repeats, warmup):
    t = {b: [] for b in fns}
    for _ in range(warmup):
        for b in fns:
            fns[b]()
    torch.cuda.synchronize()
    for _ in range(repeats):      # alternating windows
        for b in fns:
            t[b].append(window(fns[b], iters))
    rec = dict(iters_per_window=iters, repeats=repeats)
    for b, v in t.items():
        rec[b + "_us_median"] = round(statistics.median(v), 2)
        rec[b + "_us_min"], rec[b + "_us_max"] = round(min(v), 2), round(max(v), 2)
    spread = max(t["torch"]) - min(t["torch"])
    rec["torch_spread_us"] = round(spread, 2)
    rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
    rec["wins"] = bool(statistics.median(t["torch"]) - statistics.median(t["hip"]) > spread)
    return rec


def table(records):
    rows = ["| what | agents | env-steps / envs | hip µs (min-max) | torch µs (min-max) | torch spread µs | torch / hip | wins |", "|---|---|---|---|---|---|---|---|"]
    for r in records:
        rows.append("| %s | %d | %d | %.0f (%.0f-%.0f) | %.0f (%.0f-%.0f) | %.0f | %.2f | %s |" % (
            r["what"], r["agents"], r["env_steps"], r["hip_us_median"], r["hip_us_min"], r["hip_us_max"], r["torch_us_median"], r["torch_us_min"],
            r["torch_us_max"], r["torch_spread_us"], r["torch_over_hip"], "yes" if r["wins"] else "no"))
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20x128,50x128,20x4096")
    ap.add_argument("--envs", default="1,4096")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--readme", default=None, help="write the records as a markdown table to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tarmac_a2c.py needs a GPU"
    records = []

    def emit(**rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    torch.manual_seed(0)
    base = A.TarMACA2CPolicy(F_OBS, STATE, COMM, KEY).to(DEV)
    with torch.no_grad():
        base.dist.linear.weight.mul_(100.0)      # probabilities away from 1 / 2
    assert A.supported(base)
    for size in [s for s in args.sizes.split(",") if s]:
        N, B = (int(x) for x in size.split("x"))
        M = 2 * B
        gen = torch.Generator(device=DEV).manual_seed(1)
        obs = torch.rand((M, N, F_OBS), device=DEV, generator=gen) * 2 - 1
        comm = torch.randn((M, N, COMM), device=DEV, generator=gen) * 0.3
        action = torch.randint(0, 2, (M, N), device=DEV, generator=gen)
        ret = torch.randn((M, N), device=DEV, generator=gen)
        index = torch.randperm(M, device=DEV, generator=gen)[:B]
        pol = {b: copy.deepcopy(base) for b in ("hip", "torch")}
        opts = {b: torch.optim.Adam(p.parameters(), LR) for b, p in pol.items()}

        def hip_backward():
            return A.loss_backward(pol["hip"], obs, comm, action, ret, VC, EC, index=index)

        def torch_backward():
            v, a, e = A.dense_losses(pol["torch"], obs[index], comm[index], action[index], ret[index])
            opts["torch"].zero_grad()
            (v * VC + a - e * EC).backward()
            return v

        def stepper(b, backward):
            def fn():
                backward()
                nn.utils.clip_grad_norm_(pol[b].parameters(), MAX_NORM)
                opts[b].step()
            return fn

        # the two paths agree before anything is timed
        hip_backward(), torch_backward()
        grads = {b: torch.cat([p.grad.reshape(-1) for p in A._reached(q)]).clone() for b, q in pol.items()}
        diff = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
        iters = max(5, min(500, 100000 // B))
        for what, fns in (("loss backward", dict(hip=hip_backward, torch=torch_backward)),
                          ("update step", dict(hip=stepper("hip", hip_backward), torch=stepper("torch", torch_backward)))):
            emit(what=what, agents=N, env_steps=B, max_rel_diff_of_gradients=diff, **measure(fns, iters, args.repeats, args.warmup))
        del pol, opts
        torch.cuda.empty_cache()
    for E in [int(x) for x in args.envs.split(",") if x]:
        N = 20
        gen = torch.Generator(device=DEV).manual_seed(2)
        obs = torch.rand((E, N, F_OBS), device=DEV, generator=gen) * 2 - 1
        comm = torch.randn((E, N, COMM), device=DEV, generator=gen) * 0.3
        action = torch.empty(E * N, dtype=torch.uint8, device=DEV)
        a_prob = torch.empty(E * N, dtype=torch.float32, device=DEV)
        comm_out = torch.empty((E, N, COMM), device=DEV)
        fns = {b: (lambda k=(b == "hip"): base.act(obs, comm, 3, 5, action=action, a_prob=a_prob, comm_out=comm_out, kernels=k)) for b in ("hip", "torch")}
        got = {}
        for b in fns:
            _, _, v, c = fns[b]()
            got[b] = (v.clone(), c.clone())
        diff = max(float((got["hip"][i] - got["torch"][i]).abs().max() / got["torch"][i].abs().max()) for i in (0, 1))
        emit(what="act", agents=N, env_steps=E, max_rel_diff_of_value_and_comm=diff, **measure(fns, max(5, min(500, 400000 // E)), args.repeats, args.warmup))
    for path, text in ((args.out, "\n".join(json.dumps(r) for r in records) + "\n"), (args.readme, table(records) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
