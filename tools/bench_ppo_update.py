#!/usr/bin/env python3
"""One minibatch of PPO.update: mdr_amd.ppo's kernels (loss + gradient of the actor and of the critic) against torch autograd of the
reference's expressions (agents/ppo.py:148-183) on the same tensors, same GPU, same session.  The parent of this feature has no
update path: autograd is what a user runs without it, and the baseline.  HIP events after warm-up, the two backends alternating;
the median of `--repeats` windows and their spread; one JSON line per (size, network).

    python tools/bench_ppo_update.py [--rows 256,65536,4194304] [--repeats 7] [--warmup 3] [--out FILE]

Both sides start from the transition buffer and end with the six .grad of the network filled and the loss on the device; the
minibatch is the whole buffer in order (index = None: no gather on either side).  flop: 2 (F H1 + H1 H2 + H2 O) forward, the
same again for the three weight gradients and 2 H1 H2 for the input gradient of layer 2, per row; the share of the fp32
matrix peak (157.3 TF) is flop over the kernels' call time.  Per-kernel times come from `rocprofv3 --kernel-trace --stats -- python
tools/bench_ppo_update.py --only hip` in a run of its own (k_ppo_grad, k_ppo_grad_reduce).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from mdr_amd import ppo  # noqa: E402
from mdr_amd.rollout import ActorMLP, CriticMLP  # noqa: E402

DEV = "cuda:0"
F_OBS, LAYERS, CLIP = 51, (100, 100), 0.2
PEAK_FP32_MATRIX = 157.3e12


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def flop_per_row(out):
    h1, h2 = LAYERS
    fwd = 2 * (F_OBS * h1 + h1 * h2 + h2 * out)
    return fwd + 2 * (F_OBS * h1 + h1 * h2 + h2 * out) + 2 * h1 * h2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="256,65536,4194304")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ppo_update.py needs a GPU"
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for B in (int(x) for x in args.rows.split(",")):
        torch.manual_seed(0)
        gen = torch.Generator(device=DEV).manual_seed(1)
        actor, critic = ActorMLP(F_OBS, layers=LAYERS).to(DEV), CriticMLP(F_OBS, layers=LAYERS).to(DEV)
        state = torch.rand((B, F_OBS), device=DEV, generator=gen) * 2 - 1
        action = torch.randint(0, 2, (B,), device=DEV, generator=gen)
        with torch.no_grad():
            old = (actor(state).gather(1, action[:, None]).squeeze(1) * torch.exp(0.3 * torch.randn(B, device=DEV, generator=gen))).contiguous()
        target = torch.randn(B, device=DEV, generator=gen)
        adv = torch.randn(B, device=DEV, generator=gen)
        iters = max(3, min(200, int(2e6 // max(B, 1)) + 3))      # windows of comparable length at every size

        def actor_hip():
            ppo.actor_loss_backward(actor, state, action, old, adv, CLIP)

        def actor_torch():
            actor.zero_grad(set_to_none=True)
            ratio = actor(state).gather(1, action[:, None]) / old[:, None]
            a = adv[:, None]
            (-torch.min(ratio * a, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * a).mean()).backward()

        def critic_hip():
            ppo.critic_loss_backward(critic, state, target)

        def critic_torch():
            critic.zero_grad(set_to_none=True)
            F.mse_loss(target[:, None], critic(state)).backward()

        for name, out, hip, ref in (("actor", 2, actor_hip, actor_torch), ("critic", 1, critic_hip, critic_torch)):
            # the two backends agree before anything is timed
            ref()
            g_ref = torch.cat([p.grad.reshape(-1) for p in (actor if out == 2 else critic).parameters()]).clone()
            (actor if out == 2 else critic).zero_grad(set_to_none=True)
            hip()
            g_hip = torch.cat([p.grad.reshape(-1) for p in (actor if out == 2 else critic).parameters()]).clone()
            diff = float((g_hip - g_ref).abs().max() / g_ref.abs().max())
            t = {"hip": [], "torch": []}
            for _ in range(args.warmup):
                hip(), ref()
            torch.cuda.synchronize()
            for _ in range(args.repeats):      # alternating windows
                if args.only != "torch":
                    (actor if out == 2 else critic).zero_grad(set_to_none=True)
                    t["hip"].append(window(hip, iters))
                if args.only != "hip":
                    t["torch"].append(window(ref, iters))
            rec = dict(what="ppo %s loss + gradient" % name, rows=B, iters_per_window=iters, repeats=args.repeats, max_rel_diff_of_gradients=diff)
            for k, v in t.items():
                if v:
                    rec[k + "_us_median"] = round(statistics.median(v), 2)
                    rec[k + "_us_min"], rec[k + "_us_max"] = round(min(v), 2), round(max(v), 2)
            if t["hip"]:
                rec["hip_TFLOPs"] = round(B * flop_per_row(out) / statistics.median(t["hip"]) * 1e-6, 2)
                rec["hip_share_of_fp32_matrix_peak"] = round(B * flop_per_row(out) / (statistics.median(t["hip"]) * 1e-6) / PEAK_FP32_MATRIX, 4)
            if t["hip"] and t["torch"]:
                rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
            emit(**rec)
        del actor, critic, state, action, old, target, adv
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
