#!/usr/bin/env python3
"""One minibatch of PPO.update in the two precisions of mdr_amd.ppo's kernels: precision="bf16x3" (csrc/mdr_ppo_grad_bf16.hip) against
precision="fp32" (csrc/mdr_ppo_grad.hip) on the same tensors, same GPU, same session - tools/bench_ppo_update.py's method: HIP
events after warm-up, the two alternating, the median of `--repeats` windows and their range; one JSON line per (size, head).

    python tools/bench_ppo_update_bf16.py [--rows 256,65536,4194304] [--repeats 7] [--warmup 3] [--out FILE]

Both sides are the eager Python calls (actor_loss_backward / critic_loss_backward, index = None), so a small minibatch measures the
call path they share.  flop as in tools/bench_ppo_update.py (the algorithm's, not the three bf16 products' each); the share of the
fp32 matrix peak is given for both so that the two lines compare.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from mdr_amd import ppo  # noqa: E402
from mdr_amd.rollout import ActorMLP, CriticMLP  # noqa: E402
from tools.bench_ppo_update import CLIP, DEV, F_OBS, LAYERS, PEAK_FP32_MATRIX, flop_per_row, window  # noqa: E402

PRECISIONS = ("fp32", "bf16x3")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="256,65536,4194304")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ppo_update_bf16.py needs a GPU"
    lines = []
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
        calls = {"actor": lambda p: ppo.actor_loss_backward(actor, state, action, old, adv, CLIP, precision=p),
                 "critic": lambda p: ppo.critic_loss_backward(critic, state, target, precision=p)}
        for name, out in (("actor", 2), ("critic", 1)):
            net, call = (actor if out == 2 else critic), calls[name]
            grads = {}
            for p in PRECISIONS:      # the two precisions agree before anything is timed
                net.zero_grad(set_to_none=True)
                call(p)
                grads[p] = torch.cat([q.grad.reshape(-1) for q in net.parameters()]).clone()
            diff = float((grads["bf16x3"] - grads["fp32"]).abs().max() / grads["fp32"].abs().max())
            t = {p: [] for p in PRECISIONS}
            for _ in range(args.warmup):
                for p in PRECISIONS:
                    call(p)
            torch.cuda.synchronize()
            for _ in range(args.repeats):      # alternating windows
                for p in PRECISIONS:
                    t[p].append(window(lambda: call(p), iters))
            rec = dict(what="ppo %s loss + gradient" % name, rows=B, iters_per_window=iters, repeats=args.repeats,
                       max_rel_diff_of_gradients=diff)
            for p, v in t.items():
                med = statistics.median(v)
                rec[p + "_us_median"], rec[p + "_us_min"], rec[p + "_us_max"] = round(med, 2), round(min(v), 2), round(max(v), 2)
                rec[p + "_share_of_fp32_matrix_peak"] = round(B * flop_per_row(out) / (med * 1e-6) / PEAK_FP32_MATRIX, 4)
            rec["fp32_over_bf16x3"] = round(statistics.median(t["fp32"]) / statistics.median(t["bf16x3"]), 3)
            lines.append(json.dumps(rec))
            print(lines[-1], flush=True)
        del actor, critic, state, action, old, target, adv
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
