#!/usr/bin/env python3
"""One actor loss + gradient evaluation of TarMAC-PPO's update: mdr_amd.tarmac_ppo.actor_loss_backward (the kernels of
csrc/mdr_tarmac_ppo_grad.hip) against the path the parent of this feature offers on the same tensors, same GPU, same session -
``TarMACActor.forward(obs, differentiable=True)`` and ``backward()`` of the same clipped surrogate (profiles/tarmac_grad_README.md
measured it at 62.9 / 63.2 ms for the two large shapes).  F = 51, H = 64, K = 8, V = 16, c = 10, one hop.  HIP events after warm-up,
the two backends alternating; the median of ``--repeats`` windows and their spread; one JSON line per shape, and one for a whole
``TarMACPPOLearner.update`` (10 epochs of one 256-env-step minibatch) with both backends.

    python tools/bench_tarmac_ppo.py [--shapes 256x20,4096x1024,83886x50] [--repeats 5] [--warmup 2] [--only hip|torch] [--out FILE]

Both sides start from the stored env-steps and end with every reached .grad filled and the loss on the device; the minibatch is
the whole buffer in order.  flop per agent: 2 P for the forward (P the reached weights), 2 P for the weight gradients, 2 P less the
first layer for the input gradients and 2 (P - head - obs2hidden.2) for the recomputed activations; the attention is not counted.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/bench_tarmac_ppo.py --only hip` in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from mdr_amd import tarmac_ppo as tp  # noqa: E402
from mdr_amd.tarmac import TarMACActor, TarMACCritic  # noqa: E402

DEV = "cuda:0"
F_OBS, H, K, V, CLIP = 51, 64, 8, 16, 0.2
PEAK_FP32_MATRIX = 157.3e12


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def flop_per_agent():
    o2h0, hh, head0, head2 = F_OBS * H, H * H, H * (H + V), 2 * H
    proj = 3 * hh + 2 * K * H + V * H
    weights = o2h0 + hh + head0 + head2 + proj
    return 2 * weights + 2 * weights + 2 * (weights - o2h0) + 2 * (o2h0 + 3 * hh)


def surrogate(prob, action, old, adv):
    ratio = prob.gather(2, action.unsqueeze(2)).squeeze(2) / old
    return -torch.min(ratio * adv, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * adv).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256x20,4096x1024,83886x50")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tarmac_ppo.py needs a GPU"
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for B, N in (tuple(int(x) for x in s.split("x")) for s in args.shapes.split(",")):
        torch.manual_seed(0)
        gen = torch.Generator(device=DEV).manual_seed(1)
        actor = TarMACActor(F_OBS, num_key=K, num_value=V, hidden_state_size=H, number_agents_comm=10).to(DEV)
        state = torch.rand((B, N, F_OBS), device=DEV, generator=gen) * 2 - 1
        action = torch.randint(0, 2, (B, N), device=DEV, generator=gen)
        with torch.no_grad():
            old = (actor(state).gather(2, action.unsqueeze(2)).squeeze(2) * torch.exp(0.3 * torch.randn((B, N), device=DEV, generator=gen))).contiguous()
        adv = torch.randn((B, N), device=DEV, generator=gen)
        A = B * N
        iters = max(2, min(100, int(2e6 // A) + 2))

        def hip():
            tp.actor_loss_backward(actor, state, action, old, adv, CLIP)

        def ref():
            actor.zero_grad(set_to_none=True)
            surrogate(actor(state, differentiable=True), action, old, adv).backward()

        def flat():
            return torch.cat([p.grad.reshape(-1) for p in tp._params(actor)]).clone()

        ref()
        g_ref = flat()
        actor.zero_grad(set_to_none=True)
        hip()
        g_hip = flat()
        diff = float((g_hip - g_ref).abs().max() / g_ref.abs().max())
        t = {"hip": [], "torch": []}
        for _ in range(args.warmup):
            hip(), ref()
        torch.cuda.synchronize()
        for _ in range(args.repeats):      # alternating windows
            if args.only != "torch":
                actor.zero_grad(set_to_none=True)
                t["hip"].append(window(hip, iters))
            if args.only != "hip":
                t["torch"].append(window(ref, iters))
        rec = dict(what="tarmac-ppo actor loss + gradient", env_steps=B, houses=N, agents=A, iters_per_window=iters, repeats=args.repeats,
                   max_rel_diff_of_gradients=diff)
        for k, v in t.items():
            if v:
                rec[k + "_us_median"] = round(statistics.median(v), 2)
                rec[k + "_us_min"], rec[k + "_us_max"] = round(min(v), 2), round(max(v), 2)
        if t["hip"]:
            rec["hip_TFLOPs"] = round(A * flop_per_agent() / statistics.median(t["hip"]) * 1e-6, 2)
            rec["hip_share_of_fp32_matrix_peak"] = round(A * flop_per_agent() / (statistics.median(t["hip"]) * 1e-6) / PEAK_FP32_MATRIX, 4)
        if t["hip"] and t["torch"]:
            rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
        emit(**rec)
        del actor, state, action, old, adv
        torch.cuda.empty_cache()

    # a whole update: 256 stored env-steps of 20 houses, the reference's 10 epochs of one 256-row minibatch
    T, E, N = 16, 16, 20
    gen = torch.Generator(device=DEV).manual_seed(2)
    batch = {"state": torch.rand((T + 1, E * N, F_OBS), device=DEV, generator=gen) * 2 - 1,
             "action": torch.randint(0, 2, (T, E * N), device=DEV, generator=gen),
             "a_prob": 0.3 + 0.4 * torch.rand((T, E * N), device=DEV, generator=gen),
             "return": torch.randn((T, E * N), device=DEV, generator=gen)}
    rec = dict(what="TarMACPPOLearner.update", env_steps=T * E, houses=N, epochs=10, batch_size=256, repeats=args.repeats)
    t = {}
    for backend in ("hip", "torch"):
        if args.only not in (None, backend):
            continue
        torch.manual_seed(0)
        learner = tp.TarMACPPOLearner(TarMACActor(F_OBS).to(DEV), TarMACCritic(N, F_OBS).to(DEV), 1e-3, 1e-3, backend=backend)
        for _ in range(args.warmup):
            learner.update(batch)
        torch.cuda.synchronize()
        t[backend] = [window(lambda: learner.update(batch), 1) for _ in range(args.repeats)]
        rec[backend + "_us_median"] = round(statistics.median(t[backend]), 1)
        rec[backend + "_us_min"], rec[backend + "_us_max"] = round(min(t[backend]), 1), round(max(t[backend]), 1)
    if len(t) == 2:
        rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
    emit(**rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
