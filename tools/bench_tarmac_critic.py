#!/usr/bin/env python3
"""TarMAC-PPO's centralised critic step: mdr_amd.tarmac_ppo's critic kernels against torch autograd of the statements they replace
(``step_minibatch``: ``target[index] - critic(state[index])``, ``pow(delta, 2).mean(0).mean(0)``, ``zero_grad()``, ``backward()``) on
the same buffers, same GPU, same process.  HIP events after warm-up, the two paths alternating; the median of `--repeats` windows,
their minimum and maximum; one JSON line per (size, what).

    python tools/bench_tarmac_critic.py [--sizes 20x64,20x256,20x4096,50x256] [--repeats 7] [--warmup 3] [--out FILE]

Three measurements per size (agents x env-steps per minibatch; F = 51, hidden 64-64 as the reference's critic_hidden_layer_size):
  "critic backward"  value, advantage, loss and gradient of one minibatch
  "critic step"      the same + clip_grad_norm_ + Adam, as the learner runs it
  "update"           a whole ``TarMACPPOLearner.update`` - two epochs over a buffer of two minibatches - with critic_backend "hip"
                     against "torch", the actor on its kernels in both
A record's ``wins`` says whether the kernels beat autograd by more than the comparator's own run-to-run spread:
torch median - hip median > torch max - torch min.  ``critic_backend="auto"`` takes its range from the "critic step" records.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
from mdr_amd import tarmac_ppo  # noqa: E402
from mdr_amd.tarmac import TarMACActor, TarMACCritic  # noqa: E402

DEV = "cuda:0"
F_OBS, HIDDEN, MAX_NORM = 51, 64, 0.5


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
    ap.add_argument("--sizes", default="20x64,20x256,20x4096,50x256")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tarmac_critic.py needs a GPU"
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for size in args.sizes.split(","):
        N, B = (int(x) for x in size.split("x"))
        M = 2 * B
        gen = torch.Generator(device=DEV).manual_seed(1)
        states = torch.rand((M + 1, N, F_OBS), device=DEV, generator=gen) * 2 - 1
        batch = {"state": states, "action": torch.randint(0, 2, (M, N), device=DEV, generator=gen),
                 "a_prob": 0.3 + 0.4 * torch.rand((M, N), device=DEV, generator=gen), "return": torch.randn((M, N), device=DEV, generator=gen)}
        state, target = states[:M], batch["return"]
        index = torch.randperm(M, device=DEV, generator=gen)[:B]
        torch.manual_seed(0)
        critics = {b: TarMACCritic(N, F_OBS, HIDDEN).to(DEV) for b in ("hip", "torch")}
        critics["torch"].load_state_dict(critics["hip"].state_dict())
        opts = {b: torch.optim.Adam(c.parameters(), 3e-3) for b, c in critics.items()}
        assert tarmac_ppo.critic_supported(critics["hip"])

        def hip_backward():
            return tarmac_ppo.critic_loss_backward(critics["hip"], state, target, index=index)

        def torch_backward():
            delta = target[index] - critics["torch"](state[index])
            value_loss = torch.pow(delta, 2).mean(0).mean(0)
            opts["torch"].zero_grad()
            value_loss.backward()
            return value_loss

        def stepper(b, backward):
            def fn():
                backward()
                nn.utils.clip_grad_norm_(critics[b].parameters(), MAX_NORM)
                opts[b].step()
            return fn

        # the two paths agree before anything is timed
        hip_backward(), torch_backward()
        grads = {b: torch.cat([p.grad.reshape(-1) for p in c.parameters()]).clone() for b, c in critics.items()}
        diff = float((grads["hip"] - grads["torch"]).abs().max() / grads["torch"].abs().max())

        actor = TarMACActor(F_OBS).to(DEV)
        learners = {}
        for b in ("hip", "torch"):
            a, c = TarMACActor(F_OBS).to(DEV), TarMACCritic(N, F_OBS, HIDDEN).to(DEV)
            a.load_state_dict(actor.state_dict()), c.load_state_dict(critics["hip"].state_dict())
            learners[b] = tarmac_ppo.TarMACPPOLearner(a, c, 1e-3, 3e-3, ppo_update_time=2, batch_size=B, backend="hip", critic_backend=b)

        whats = (("critic backward", dict(hip=hip_backward, torch=torch_backward), max(5, min(1000, 200000 // B))),
                 ("critic step", dict(hip=stepper("hip", hip_backward), torch=stepper("torch", torch_backward)), max(5, min(1000, 200000 // B))),
                 ("update", {b: (lambda l=learners[b]: l.update(batch, seed=0, nb_houses=N)) for b in ("hip", "torch")}, max(2, min(50, 20000 // B))))
        for what, fns, iters in whats:
            t = {b: [] for b in fns}
            for _ in range(args.warmup):
                for b in fns:
                    fns[b]()
            torch.cuda.synchronize()
            for _ in range(args.repeats):      # alternating windows
                for b in fns:
                    t[b].append(window(fns[b], iters))
            rec = dict(what=what, agents=N, env_steps=B, joint_inputs=N * F_OBS, hidden=HIDDEN, iters_per_window=iters, repeats=args.repeats,
                       max_rel_diff_of_gradients=diff)
            for b, v in t.items():
                rec[b + "_us_median"] = round(statistics.median(v), 2)
                rec[b + "_us_min"], rec[b + "_us_max"] = round(min(v), 2), round(max(v), 2)
            spread = max(t["torch"]) - min(t["torch"])
            rec["torch_spread_us"] = round(spread, 2)
            rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
            rec["wins"] = bool(statistics.median(t["torch"]) - statistics.median(t["hip"]) > spread)
            emit(**rec)
        del learners, critics, opts
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
