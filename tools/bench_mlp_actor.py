#!/usr/bin/env python3
"""Acting with the 256-256 actor: FusedMLPActor.sample (one kernel, csrc/mdr_mlp_actor.hip) against what collect_maddpg_transitions runs
without it - ``actor(rows)`` under ``torch.no_grad()`` + ``mdr_logits_sample`` - on the same rows, same GPU, same session.  HIP events
after warm-up, the two paths alternating; the median of `--repeats` windows and their spread; one JSON line per batch.

    python tools/bench_mlp_actor.py [--repeats 7] [--warmup 3] [--only hip|torch] [--precision fp32,bf16x3] [--cases 51:1x20,...] [--out FILE]

Batches (features : envs x houses), hidden 256-256: 51:1x20, 51:64x50, 51:4096x20, 51:4096x1024 and 121:4096x1024.  Before anything is
timed the worst difference between the two paths' probabilities is printed.  ``floor_us`` is the batch's FLOPs - 2 (F H1 + H1 H2 + 2 H2)
per agent, counted from the shapes - at the 157.3 TFLOP/s fp32 matrix peak of the MI355X, ``floor_share`` that over the kernel path's
median window (launch overhead included: at the small batches the share is that of an empty launch).
``--precision fp32,bf16x3`` times ``FusedMLPActor(precision="bf16x3")`` (csrc/mdr_mlp_actor_bf16.hip) as a third path in the same
alternating windows: ``hip_bf16x3_*``, its floor - three bf16 products of 32 k at 16 cycles against eight fp32 k-steps of 4 at 32
cycles, 3/16 of ``floor_us`` - and ``fp32_over_bf16x3`` with ``spread_us``, the wider of the two kernels' max - min.
Per-kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_mlp_actor.py --only hip` in a run of its own.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from mdr_amd import _native as nat  # noqa: E402
from mdr_amd.maddpg import DDPGNetworkMLP  # noqa: E402
from mdr_amd.mlp_actor import FusedMLPActor  # noqa: E402

DEV = "cuda:0"
HIDDEN = 256
PEAK_FP32_MATRIX = 157.3e12
CASES = "51:1x20,51:64x50,51:4096x20,51:4096x1024,121:4096x1024"


def flops(A, F, H1, H2):
    return 2.0 * A * (F * H1 + H1 * H2 + H2 * 2)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=CASES)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--precision", default="fp32", help="comma-separated precisions of the kernel path: fp32, bf16x3")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    precisions = args.precision.split(",")
    assert precisions and all(p in ("fp32", "bf16x3") for p in precisions), "--precision takes fp32 and bf16x3"
    hip_paths = {"hip" if p == "fp32" else "hip_" + p: p for p in precisions}      # path name -> precision
    assert torch.cuda.is_available(), "bench_mlp_actor.py needs a GPU"
    lib = nat.load()
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    paths = [b for b in (*hip_paths, "torch") if args.only in (None, "hip" if b in hip_paths else b)]
    for case in args.cases.split(","):
        F, shape = case.split(":")
        F, (E, N) = int(F), (int(x) for x in shape.split("x"))
        A = E * N
        torch.manual_seed(0)
        actor = DDPGNetworkMLP(F, 2, HIDDEN).to(DEV)
        with torch.no_grad():
            actor.fc[2].weight.mul_(8.0)      # probabilities away from 1/2
        rows = torch.rand((A, F), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) * 2 - 1
        fused = FusedMLPActor(actor)
        split = FusedMLPActor(actor, precision="bf16x3")
        act = {b: torch.empty(A, dtype=torch.uint8, device=DEV) for b in ("hip", "hip_bf16x3", "torch")}
        a_prob = torch.empty(A, dtype=torch.float32, device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def hip(probs=None):
            return fused.sample(rows, 5, 7, action=act["hip"], a_prob=a_prob)

        def hip_bf16x3(probs=None):
            return split.sample(rows, 5, 7, action=act["hip_bf16x3"], a_prob=a_prob)

        def torch_path(probs=None):      # rollout.collect_maddpg_transitions, actor_backend="torch"
            with torch.no_grad():
                logits = actor(rows).contiguous()
            rc = lib.mdr_logits_sample(C.c_void_p(logits.data_ptr()), logits.stride(0), A, C.c_uint64(5), C.c_uint64(7), None, 0,
                                       C.c_void_p(act["torch"].data_ptr()), None, C.c_void_p(probs.data_ptr()) if probs is not None else None, stream)
            assert rc == 0

        diff = flips = None
        if "hip" in paths and "torch" in paths:      # the two paths agree before anything is timed
            p_t = torch.empty((A, 2), dtype=torch.float32, device=DEV)
            torch_path(p_t)
            _, _, p_h = fused.sample(rows, 5, 7, action=act["hip"], want_probs=True)
            diff = float((p_h - p_t).abs().max())
            flips = int((act["hip"] != act["torch"]).sum())
            print("# %s: worst |p_hip - p_torch| = %.3e, %d of %d actions differ, p0 in [%.3f, %.3f]"
                  % (case, diff, flips, A, float(p_h[:, 0].min()), float(p_h[:, 0].max())), flush=True)
            del p_t, p_h
        diff_split = None
        if "hip" in paths and "hip_bf16x3" in paths:
            _, _, p_h = fused.sample(rows, 5, 7, action=act["hip"], want_probs=True)
            _, _, p_s = split.sample(rows, 5, 7, action=act["hip_bf16x3"], want_probs=True)
            diff_split = float((p_h - p_s).abs().max())
            print("# %s: worst |p_fp32 - p_bf16x3| = %.3e, %d of %d actions differ" % (case, diff_split, int((act["hip"] != act["hip_bf16x3"]).sum()), A), flush=True)
            del p_h, p_s
        fns = {"hip": hip, "hip_bf16x3": hip_bf16x3, "torch": torch_path}
        iters = max(3, min(200, 2000000 // A + 3))
        t = {b: [] for b in paths}
        for _ in range(args.warmup):
            for b in paths:
                fns[b]()
        torch.cuda.synchronize()
        for _ in range(args.repeats):      # alternating windows
            for b in paths:
                t[b].append(window(fns[b], iters))
        floor_us = flops(A, F, HIDDEN, HIDDEN) / PEAK_FP32_MATRIX * 1e6
        rec = dict(what="act", features=F, hidden=[HIDDEN, HIDDEN], envs=E, houses=N, agents=A, iters_per_window=iters, repeats=args.repeats,
                   max_abs_diff_of_probs=diff, actions_that_differ=flips, flop=flops(A, F, HIDDEN, HIDDEN), floor_us=round(floor_us, 3))
        for b, v in t.items():
            rec[b + "_us_median"] = round(statistics.median(v), 2)
            rec[b + "_us_min"], rec[b + "_us_max"] = round(min(v), 2), round(max(v), 2)
        if "hip" in t:
            rec["floor_share"] = round(floor_us / statistics.median(t["hip"]), 4)
        if "hip_bf16x3" in t:
            rec["bf16x3_floor_us"] = round(floor_us * 3.0 / 16.0, 3)
            rec["bf16x3_floor_share"] = round(floor_us * 3.0 / 16.0 / statistics.median(t["hip_bf16x3"]), 4)
            rec["max_abs_diff_fp32_bf16x3"] = diff_split
        if "hip" in t and "hip_bf16x3" in t:
            rec["fp32_over_bf16x3"] = round(statistics.median(t["hip"]) / statistics.median(t["hip_bf16x3"]), 3)
            rec["spread_us"] = round(max(max(t[b]) - min(t[b]) for b in ("hip", "hip_bf16x3")), 2)
        if "hip" in t and "torch" in t:
            rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
        emit(**rec)
        del actor, rows, fused, split, act, a_prob
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
