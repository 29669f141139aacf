#!/usr/bin/env python3
"""MAPPO's centralised critic step: mdr_amd.mappo.joint_critic_loss_backward (loss + gradient of Critic(F + N - 1), the others' actions
gathered from `action` inside the kernel) against torch autograd of the reference's expressions (agents/mappo.py:87, 113-116) on a
materialised int64 others_actions tensor - same tensors, same GPU, same session.  The parent of this feature has no MAPPO update:
autograd on rollout.others_actions() is what a user ran, and the baseline.  HIP events after warm-up, the two backends alternating;
the median of `--repeats` windows and their spread; one JSON line per (size, shape).  Then a whole ten-epoch MAPPOLearner.update at
the reference's 256 steps x 20 agents on either backend.

    python tools/bench_mappo_update.py [--rows 256,65536,4194304] [--repeats 7] [--warmup 3] [--out FILE]

Both sides start from the transition buffer and end with the six .grad of the critic filled and the loss on the device; the
minibatch is the whole buffer in order (index = None).  The autograd side is given others_actions ready-made: building it is not in
its time, only the cat and the int64 -> float conversion mappo.py:87 performs per minibatch are.  flop per row: 2 (J H1 + H1 H2 + H2)
forward, the same again for the three weight gradients and 2 H1 H2 for the input gradient of layer 2.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from mdr_amd import mappo  # noqa: E402
from mdr_amd.rollout import ActorMLP, CriticMLP, others_actions  # noqa: E402

DEV = "cuda:0"
SHAPES = ((51, 20, (100, 100)), (51, 50, (100, 100)))      # (state features, agents, hidden layers)
PEAK_FP32_MATRIX = 157.3e12


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def flop_per_row(J, layers):
    h1, h2 = layers
    return 4 * (J * h1 + h1 * h2 + h2) + 2 * h1 * h2


def stats(rec, name, v):
    rec[name + "_median"] = round(statistics.median(v), 2)
    rec[name + "_min"], rec[name + "_max"] = round(min(v), 2), round(max(v), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="256,65536,4194304")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--no-learner", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mappo_update.py needs a GPU"
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for rows in (int(x) for x in args.rows.split(",")):
        for F_OBS, N, layers in SHAPES:
            B = (rows + N - 1) // N * N      # whole env-steps
            J = F_OBS + N - 1
            torch.manual_seed(0)
            gen = torch.Generator(device=DEV).manual_seed(1)
            critic = CriticMLP(J, layers=layers).to(DEV)
            state = torch.rand((B, F_OBS), device=DEV, generator=gen) * 2 - 1
            action = torch.randint(0, 2, (B,), device=DEV, generator=gen)
            target = torch.randn(B, device=DEV, generator=gen)
            others = others_actions(action.view(1, B), B // N, N).view(B, N - 1)      # int64, as the reference's buffer holds it
            iters = max(3, min(200, int(2e6 // max(B, 1)) + 3))      # windows of comparable length at every size

            def hip():
                mappo.joint_critic_loss_backward(critic, state, action, target, nb_agents=N)

            def ref():
                critic.zero_grad(set_to_none=True)
                F.mse_loss(target[:, None], critic(torch.cat((state, others), dim=1))).backward()

            # the two backends agree before anything is timed
            ref()
            g_ref = torch.cat([p.grad.reshape(-1) for p in critic.parameters()]).clone()
            critic.zero_grad(set_to_none=True)
            hip()
            g_hip = torch.cat([p.grad.reshape(-1) for p in critic.parameters()]).clone()
            diff = float((g_hip - g_ref).abs().max() / g_ref.abs().max())
            t = {"hip": [], "torch": []}
            for _ in range(args.warmup):
                hip(), ref()
            torch.cuda.synchronize()
            for _ in range(args.repeats):      # alternating windows
                if args.only != "torch":
                    critic.zero_grad(set_to_none=True)
                    t["hip"].append(window(hip, iters))
                if args.only != "hip":
                    t["torch"].append(window(ref, iters))
            rec = dict(what="mappo joint critic loss + gradient", rows=B, num_state=F_OBS, nb_agents=N, joint_inputs=J, hidden=list(layers),
                       iters_per_window=iters, repeats=args.repeats, max_rel_diff_of_gradients=diff,
                       others_actions_bytes_per_transition=8 * (N - 1))
            for k, v in t.items():
                if v:
                    stats(rec, k + "_us", v)
            if t["hip"]:
                rate = B * flop_per_row(J, layers) / (statistics.median(t["hip"]) * 1e-6)
                rec["hip_TFLOPs"] = round(rate * 1e-12, 2)
                rec["hip_share_of_fp32_matrix_peak"] = round(rate / PEAK_FP32_MATRIX, 4)
            if t["hip"] and t["torch"]:
                rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
            emit(**rec)
            del critic, state, action, target, others
            torch.cuda.empty_cache()

    if not args.no_learner:
        # a whole MAPPO.update: ten epochs over 256 steps x 20 agents in minibatches of 256 (config MAPPO_prop), both backends
        F_OBS, N, layers = SHAPES[0]
        T = 256
        gen = torch.Generator(device=DEV).manual_seed(2)
        torch.manual_seed(0)
        actor0, critic0 = ActorMLP(F_OBS, layers=layers).to(DEV), CriticMLP(F_OBS + N - 1, layers=layers).to(DEV)
        batch = dict(state=torch.rand((T + 1, N, F_OBS), device=DEV, generator=gen) * 2 - 1,
                     action=torch.randint(0, 2, (T, N), device=DEV, generator=gen))
        with torch.no_grad():
            p = actor0(batch["state"][:T].reshape(-1, F_OBS)).gather(1, batch["action"].reshape(-1, 1)).view(T, N)
        batch["a_prob"] = (p * torch.exp(0.1 * torch.randn((T, N), device=DEV, generator=gen))).contiguous()
        batch["return"] = torch.randn((T, N), device=DEV, generator=gen)
        batch["others_actions"] = others_actions(batch["action"], 1, N)
        prop = dict(lr_actor=1e-3, lr_critic=3e-3, clip_param=0.2, max_grad_norm=0.5, ppo_update_time=10, batch_size=256)
        learners = {}
        for backend in ("hip", "torch"):
            actor, critic = ActorMLP(F_OBS, layers=layers).to(DEV), CriticMLP(F_OBS + N - 1, layers=layers).to(DEV)
            actor.load_state_dict(actor0.state_dict()), critic.load_state_dict(critic0.state_dict())
            learners[backend] = mappo.MAPPOLearner.from_config(prop, actor, critic, backend=backend)
        t = {"hip": [], "torch": []}
        count = 0
        for _ in range(1):
            for lrn in learners.values():
                count = lrn.update(batch, seed=0)[2]
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for backend, lrn in learners.items():
                if args.only in (None, backend):
                    t[backend].append(window(lambda: lrn.update(batch, seed=0), 1) * 1e-3)      # ms
        rec = dict(what="MAPPOLearner.update", steps=T, nb_agents=N, transitions=T * N, epochs=10, batch_size=256, minibatches=count,
                   repeats=args.repeats)
        for k, v in t.items():
            if v:
                stats(rec, k + "_ms", v)
        if t["hip"] and t["torch"]:
            rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
        emit(**rec)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
