#!/usr/bin/env python
"""Observe -> act for the fused TarMAC actor against the path it replaces, on one GPU: per step

    rows            env.obs_vector("rows", out=scratch)   + fused.sample       (states not kept)
    rows_kept       env.obs_vector("rows", out=states[t]) + fused.sample       (states kept)
    observe         fused.sample_env(env)
    observe_kept    fused.sample_env(env, rows_out=states[t])

timed with HIP events after warm-up, alternating the four in every round, and the step of ``collect_tarmac_rollout`` (observation,
actor and ``env.step``) with ``store_states`` on / off and ``observe_act`` on / off by a host clock around a synchronised rollout.
One JSON line per record.  ``--trace``: a short untimed run of the four variants for ``rocprofv3 --kernel-trace --stats -- python
tools/bench_tarmac_observe.py --trace ...`` (per-kernel times: the kernels of the variants differ by name; no end-to-end figure is
taken under the profiler)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

DEV = "cuda:0"


def emit(**kw):
    print(json.dumps(kw), flush=True)


def make_env(E, N):
    import mdr_amd
    cfg = mdr_amd.default_config()
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = N
    cfg["default_env_prop"]["power_grid_prop"]["base_power_mode"] = "constant"
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = "big_noise"
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device=DEV, seed=3)
    env.reset(episode=0)
    env.set_obs_planes(False)
    g = torch.Generator(device="cpu").manual_seed(1)
    for _ in range(6):
        env.step((torch.rand((E, N), generator=g) < 0.5).to(torch.uint8).to(DEV))
    return env


def make_actor(hops, precision):
    from mdr_amd.tarmac import FusedTarMACActor, TarMACActor
    torch.manual_seed(11)
    actor = TarMACActor(51, num_key=8, num_value=16, hidden_state_size=64, number_agents_comm=10, num_hops=hops)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name.endswith("weight"):
                p.mul_(2.0)
    return FusedTarMACActor.from_module(actor.to(DEV), precision)


def variants(env, fused, states, scratch, action, a_prob):
    E, N = env.nb_envs, env.nb_houses

    def rows():
        fused.sample(env.obs_vector("rows", out=scratch), 7, 3, action=action, a_prob=a_prob)

    def rows_kept():
        fused.sample(env.obs_vector("rows", out=states.view(E, N, 51)), 7, 3, action=action, a_prob=a_prob)

    def observe():
        fused.sample_env(env, 7, 3, action=action, a_prob=a_prob)

    def observe_kept():
        fused.sample_env(env, 7, 3, action=action, a_prob=a_prob, rows_out=states)

    return [("rows", rows), ("rows_kept", rows_kept), ("observe", observe), ("observe_kept", observe_kept)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--houses", type=int, default=1024)
    ap.add_argument("--hops", type=int, default=1)
    ap.add_argument("--precision", default="both", choices=["fp32", "bf16x3", "both"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rollout-steps", type=int, default=6)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tarmac_observe needs the GPU: no timing is taken without one")
    from mdr_amd.rollout import collect_tarmac_rollout
    E, N = args.envs, args.houses
    A = E * N
    env = make_env(E, N)
    states = torch.empty((A, 51), dtype=torch.float32, device=DEV)
    scratch = torch.empty((E, N, 51), dtype=torch.float32, device=DEV)
    action = torch.empty(A, dtype=torch.uint8, device=DEV)
    a_prob = torch.empty(A, dtype=torch.float32, device=DEV)
    for precision in (["fp32", "bf16x3"] if args.precision == "both" else [args.precision]):
        fused = make_actor(args.hops, precision)
        todo = variants(env, fused, states, scratch, action, a_prob)
        outs = {}
        for name, fn in todo:      # warm-up, and the outputs must not depend on the path
            fn()
            fn()
            outs[name] = (action.clone(), a_prob.clone())
        torch.cuda.synchronize()
        same = all(torch.equal(outs["rows"][0], o[0]) and torch.equal(outs["rows"][1], o[1]) for o in outs.values())
        if args.trace:
            for name, fn in todo:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            emit(what="trace", envs=E, houses=N, hops=args.hops, precision=precision, outputs_equal=same, launches_per_variant=3)
            continue
        best = {name: [] for name, _ in todo}
        for _ in range(args.rounds):
            for name, fn in todo:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.iters):
                    fn()
                t1.record()
                t1.synchronize()
                best[name].append(t0.elapsed_time(t1) * 1e3 / args.iters)
        emit(what="sample_step_us", envs=E, houses=N, agents=A, hops=args.hops, precision=precision, outputs_equal=same, iters=args.iters,
             **{name: {"mean": round(sum(v) / len(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} for name, v in best.items()})
        T = args.rollout_steps
        for store in (False, True):
            rec = {}
            for observe_act in (False, True, False, True):
                collect_tarmac_rollout(env, fused, 1, store_states=store, observe_act=observe_act)      # warm-up (allocations)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                collect_tarmac_rollout(env, fused, T, store_states=store, observe_act=observe_act)
                torch.cuda.synchronize()
                rec.setdefault("observe" if observe_act else "rows", []).append(round((time.perf_counter() - t0) * 1e6 / T, 1))
                torch.cuda.empty_cache()
            emit(what="rollout_step_us", envs=E, houses=N, hops=args.hops, precision=precision, store_states=store, steps=T, **rec)


if __name__ == "__main__":
    main()
