#!/usr/bin/env python
"""Per-step time of the fused TarMAC actor for a kernel form the other tools do not reach: tools/bench_tarmac.py and
tools/bench_tarmac_observe.py run the reference's sizes (H = 64, K = 8, V = 16), which select the exact forms of
csrc/mdr_tarmac_mlp.hip / csrc/mdr_tarmac_mlp_bf16.hip; any other covered shape selects the general forms.

    python tools/bench_tarmac_forms.py [--envs 4096] [--houses 1024] [--hidden 48] [--keys 16] [--values 32] [--hops 2]
                                       [--precision fp32|bf16x3|both] [--rounds 5] [--iters 10]

Times ``sample`` on observation rows (``rows``), ``sample_env`` (``observe``) and ``sample_env`` with ``rows_out`` (``observe_kept``) on
the env of tools/bench_tarmac_observe.py, F = 51, with HIP events after warm-up, the three alternating in every round.  One JSON line
per precision and path with the per-round means in microseconds, their mean, min and max, and ``lib``: the library that ran
(``MDR_HIP_LIB`` selects a ``build_variant``, so that two builds can be measured side by side in alternating processes)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench_tarmac_observe as bo  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--houses", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=48)
    ap.add_argument("--keys", type=int, default=16)
    ap.add_argument("--values", type=int, default=32)
    ap.add_argument("--hops", type=int, default=2)
    ap.add_argument("--precision", default="both", choices=["fp32", "bf16x3", "both"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tarmac_forms needs the GPU: no timing is taken without one")
    from mdr_amd.tarmac import FusedTarMACActor, TarMACActor
    E, N = args.envs, args.houses
    A = E * N
    env = bo.make_env(E, N)
    obs = torch.randn((E, N, 51), device=DEV)
    states = torch.empty((A, 51), device=DEV)
    action = torch.empty(A, dtype=torch.uint8, device=DEV)
    a_prob = torch.empty(A, device=DEV)
    blocks = lambda n: (n + 15) // 16      # noqa: E731  (the launcher's rule, csrc/mdr_tarmac_mlp.h run_chain)
    form = "exact" if blocks(args.hidden) == 4 and blocks(args.values) == 1 and (args.hops == 1 or blocks(args.hidden + args.values) == 5) else "general"
    for precision in (["fp32", "bf16x3"] if args.precision == "both" else [args.precision]):
        torch.manual_seed(11)
        actor = TarMACActor(51, num_key=args.keys, num_value=args.values, hidden_state_size=args.hidden, number_agents_comm=10, num_hops=args.hops)
        fused = FusedTarMACActor.from_module(actor.to(DEV), precision)
        paths = [("rows", lambda: fused.sample(obs, 7, 3, action=action, a_prob=a_prob)),
                 ("observe", lambda: fused.sample_env(env, 7, 3, action=action, a_prob=a_prob)),
                 ("observe_kept", lambda: fused.sample_env(env, 7, 3, action=action, a_prob=a_prob, rows_out=states))]
        for _, fn in paths:
            fn()
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in paths}
        for _ in range(args.rounds):
            for name, fn in paths:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    fn()
                t1.record()
                t1.synchronize()
                times[name].append(round(t0.elapsed_time(t1) * 1e3 / args.iters, 1))
        for name, v in times.items():
            print(json.dumps(dict(what="forms_step_us", lib=os.path.basename(os.environ.get("MDR_HIP_LIB", "libmdr_hip.so")), envs=E, houses=N,
                                  hidden=args.hidden, keys=args.keys, values=args.values, hops=args.hops, form=form, precision=precision, path=name,
                                  us=v, mean=round(sum(v) / len(v), 1), min=min(v), max=max(v))), flush=True)
        del fused
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
