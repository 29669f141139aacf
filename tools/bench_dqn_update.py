#!/usr/bin/env python3
"""One update of DQN / DDQN: mdr_amd.dqn's kernels against torch autograd of the reference's expressions (agents/dqn.py:84-146) on the
same replay buffer, same GPU, same session.  The parent of this feature has no DQN update: autograd is what a user runs without it,
and the baseline.  HIP events after warm-up, the two backends alternating; the median of `--repeats` windows and their spread; one
JSON line per (size, mode, what).

    python tools/bench_dqn_update.py [--rows 256,65536] [--repeats 7] [--warmup 3] [--out FILE]

Two measurements per size and mode:
  "update"   a whole ``DQNLearner.update``: sample -> TD target -> loss, backward, clamp -> Adam -> target blend
  "target + gradient"   ``DQNLearner.loss_backward`` on a fixed index tensor: what the kernels replace (torch: the gathers, two or three
             forward passes, one backward and the six clamps)
The buffer holds 2^19 transitions of the reference's network (F = 51, hidden 100-100); the minibatch is `rows` sampled positions.
Per-kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_dqn_update.py --only hip` in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from mdr_amd import dqn  # noqa: E402

DEV = "cuda:0"
F_OBS, LAYERS, CAPACITY = 51, (100, 100), 524288


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def learner_for(backend, B, double, state):
    torch.manual_seed(0)
    lrn = dqn.DQNLearner(dqn.QNetworkMLP(F_OBS, layers=LAYERS).to(DEV), 1e-3, buffer_capacity=CAPACITY, batch_size=B, double=double,
                         backend=backend)
    lrn.buffer.push(*state)
    return lrn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="256,65536")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_dqn_update.py needs a GPU"
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    gen = torch.Generator(device=DEV).manual_seed(1)
    state = (torch.rand((CAPACITY, F_OBS), device=DEV, generator=gen) * 2 - 1, torch.randint(0, 2, (CAPACITY,), device=DEV, generator=gen),
             torch.randn(CAPACITY, device=DEV, generator=gen), torch.rand((CAPACITY, F_OBS), device=DEV, generator=gen) * 2 - 1)
    backends = [b for b in ("hip", "torch") if args.only in (None, b)]
    for B in (int(x) for x in args.rows.split(",")):
        iters = max(3, min(200, int(2e6 // max(B, 1)) + 3))      # windows of comparable length at every size
        for double in (False, True):
            lrn = {b: learner_for(b, B, double, state) for b in backends}
            index = next(iter(lrn.values())).sample(0)
            diff = None
            if len(backends) == 2:      # the two backends agree before anything is timed
                grads = {}
                for b in backends:
                    lrn[b].loss_backward(index)
                    grads[b] = torch.cat([p.grad.reshape(-1) for p in lrn[b].policy_net.parameters()]).clone()
                diff = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())
            for what, fns in (("update", {b: lrn[b].update for b in backends}),
                              ("target + gradient", {b: (lambda l=lrn[b]: l.loss_backward(index)) for b in backends})):
                t = {b: [] for b in backends}
                for _ in range(args.warmup):
                    for b in backends:
                        fns[b]()
                torch.cuda.synchronize()
                for _ in range(args.repeats):      # alternating windows
                    for b in backends:
                        t[b].append(window(fns[b], iters))
                rec = dict(what="%s %s" % ("ddqn" if double else "dqn", what), rows=B, iters_per_window=iters, repeats=args.repeats,
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
