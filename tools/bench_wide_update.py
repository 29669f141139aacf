#!/usr/bin/env python3
"""The update step on observations with message columns (81 / 91 / 121 features): the wide entry points (`wide=True`, mdr_*_wide)
against torch autograd of the reference's expressions on the same tensors, same GPU, same session.  Without `wide=True` - and on
every commit before it - autograd is what a run with a message flag gets.  HIP events after warm-up, the backends alternating; the
median of `--repeats` windows and their spread; one JSON line per measurement.

    python tools/bench_wide_update.py heads    [--rows 1,16,64,256,65536] [--repeats 7] [--warmup 3] [--out FILE]
    python tools/bench_wide_update.py learners [--envs 4096] [--repeats 3] [--out FILE]

heads: one minibatch of the actor, critic and Huber heads at (81 | 91 | 121, 100, 100) and of the joint critic at 110 inputs (91
features, 20 agents); both sides start from the transition buffer and end with the six .grad filled and the loss on the device.
learners: a whole PPOLearner.update (one epoch over envs x 20 agents x 8 steps in minibatches of 256) and DQNLearner.update
(minibatches of 256 from a buffer holding those transitions) at 121 features: backend="torch", and with `wide=True` backend="hip"
eager and graph=True.  On a tree without the wide entry points the script times the torch side alone (`--only torch` is implied).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from mdr_amd import dqn, mappo, ppo  # noqa: E402
from mdr_amd.optim import FusedAdam  # noqa: E402
from mdr_amd.rollout import ActorMLP, CriticMLP  # noqa: E402

DEV = "cuda:0"
LAYERS, CLIP, AGENTS = (100, 100), 0.2, 20
HAS_WIDE = hasattr(ppo, "MAX_STATE_WIDE")


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def stats(rec, key, v):
    rec[key + "_median"] = round(statistics.median(v), 2)
    rec[key + "_min"], rec[key + "_max"] = round(min(v), 2), round(max(v), 2)
    rec[key + "_windows"] = [round(x, 2) for x in v]


def flat_grad(net):
    return torch.cat([p.grad.reshape(-1) for p in net.parameters()]).clone()


def heads(args, emit):
    only_torch = args.only == "torch" or not HAS_WIDE
    for B in (int(x) for x in args.rows.split(",")):
        for width, head in [(f, h) for f in (81, 91, 121) for h in ("actor", "critic", "huber")] + [(91, "joint")]:
            torch.manual_seed(0)
            gen = torch.Generator(device=DEV).manual_seed(1)
            rows = -(-B // AGENTS) * AGENTS if head == "joint" else B      # whole env-steps
            inputs = width + (AGENTS - 1 if head == "joint" else 0)
            net = {"actor": ActorMLP, "critic": CriticMLP, "joint": CriticMLP, "huber": dqn.QNetworkMLP}[head](inputs, layers=LAYERS).to(DEV)
            state = torch.rand((rows, width), device=DEV, generator=gen) * 2 - 1
            action = torch.randint(0, 2, (rows,), device=DEV, generator=gen)
            target = torch.randn(rows, device=DEV, generator=gen)
            adv = torch.randn(rows, device=DEV, generator=gen)
            others = mappo.gather_others(action, AGENTS) if head == "joint" else None
            with torch.no_grad():
                old = (net(state).gather(1, action[:, None]).squeeze(1) * torch.exp(0.3 * torch.randn(rows, device=DEV, generator=gen))).contiguous() \
                    if head == "actor" else None
            iters = max(3, min(200, int(2e6 // max(rows, 1)) + 3))      # windows of comparable length at every size

            def hip():
                if head == "actor":
                    ppo.actor_loss_backward(net, state, action, old, adv, CLIP, wide=True)
                elif head == "critic":
                    ppo.critic_loss_backward(net, state, target, wide=True)
                elif head == "huber":
                    dqn.q_loss_backward(net, state, action, target, grad_clamp=1.0, wide=True)
                else:
                    mappo.joint_critic_loss_backward(net, state, action, target, nb_agents=AGENTS, wide=True)

            def ref():
                net.zero_grad(set_to_none=True)
                if head == "actor":
                    ratio = net(state).gather(1, action[:, None]) / old[:, None]
                    a = adv[:, None]
                    (-torch.min(ratio * a, torch.clamp(ratio, 1 - CLIP, 1 + CLIP) * a).mean()).backward()
                elif head == "critic":
                    F.mse_loss(target[:, None], net(state)).backward()
                elif head == "huber":
                    torch.nn.SmoothL1Loss()(net(state).gather(1, action[:, None]), target[:, None]).backward()
                    for p in net.parameters():
                        p.grad.clamp_(-1.0, 1.0)
                else:
                    F.mse_loss(target[:, None], net(torch.cat((state, others.float()), 1))).backward()

            rec = dict(what="%s loss + gradient" % head, features=width, inputs=inputs, rows=rows, iters_per_window=iters, repeats=args.repeats)
            ref()
            if not only_torch:      # the two backends agree before anything is timed
                g_ref = flat_grad(net)
                net.zero_grad(set_to_none=True)
                hip()
                rec["max_rel_diff_of_gradients"] = float((flat_grad(net) - g_ref).abs().max() / g_ref.abs().max())
            t = {"hip": [], "torch": []}
            for _ in range(args.warmup):
                if not only_torch:
                    hip()
                ref()
            torch.cuda.synchronize()
            for _ in range(args.repeats):      # alternating windows
                if not only_torch:
                    net.zero_grad(set_to_none=True)
                    t["hip"].append(window(hip, iters))
                if args.only != "hip":
                    t["torch"].append(window(ref, iters))
            for k, v in t.items():
                if v:
                    stats(rec, k + "_us", v)
            if t["hip"] and t["torch"]:
                rec["torch_over_hip"] = round(statistics.median(t["torch"]) / statistics.median(t["hip"]), 3)
                rec["hip_faster_in_every_repeat"] = max(t["hip"]) < min(t["torch"])
            emit(**rec)


def learners(args, emit):
    width, T, A = 121, 8, args.envs * AGENTS
    gen = torch.Generator(device=DEV).manual_seed(2)
    batch = dict(state=torch.rand((T + 1, A, width), device=DEV, generator=gen) * 2 - 1, action=torch.randint(0, 2, (T, A), device=DEV, generator=gen),
                 a_prob=0.2 + 0.6 * torch.rand((T, A), device=DEV, generator=gen), reward=torch.randn((T, A), device=DEV, generator=gen),
                 **{"return": torch.randn((T, A), device=DEV, generator=gen)})
    modes = [("torch", dict(backend="torch"))]
    if HAS_WIDE and args.only != "torch":
        modes += [("hip wide", dict(backend="hip", wide=True, optimizer=FusedAdam, sampler="philox")),
                  ("hip wide graph", dict(backend="hip", wide=True, optimizer=FusedAdam, graph=True))]

    def ppo_learner(kw):
        torch.manual_seed(0)
        kw = dict(kw, graph_max_minibatches=1 << 20) if kw.get("graph") else kw      # one graph of the whole epoch
        return ppo.PPOLearner(ActorMLP(width, layers=LAYERS).to(DEV), CriticMLP(width, layers=LAYERS).to(DEV), 1e-3, 3e-3, batch_size=256,
                              ppo_update_time=1, **kw)

    def dqn_learner(kw):
        torch.manual_seed(0)
        L = dqn.DQNLearner(dqn.QNetworkMLP(width, layers=LAYERS).to(DEV), 1e-3, batch_size=256, **kw)
        L.store(batch)
        return L

    for what, make, run, per in (("PPOLearner.update, one epoch of %d minibatches of 256" % -(-T * A // 256), ppo_learner,
                                  lambda L, i: L.update(batch, seed=i), 1),
                                 ("DQNLearner.update, minibatch of 256", dqn_learner, lambda L, i: L.update(seed=i), 100)):
        made = [(name, make(kw)) for name, kw in modes]
        t = {name: [] for name, _ in made}
        for name, L in made:      # warm-up: code objects, the capture
            run(L, 0)
        torch.cuda.synchronize()
        for r in range(args.repeats):      # alternating
            for name, L in made:
                count = [0]

                def step():
                    count[0] += 1
                    run(L, 1 + r * per + count[0])
                t[name].append(window(step, per) / 1e3)      # ms per update
        rec = dict(what=what, features=width, transitions=T * A, updates_per_window=per, repeats=args.repeats)
        for name, v in t.items():
            stats(rec, name.replace(" ", "_") + "_ms", v)
        emit(**rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("heads", "learners"))
    ap.add_argument("--rows", default="1,16,64,256,65536")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("hip", "torch"), default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats is None:
        args.repeats = 7 if args.mode == "heads" else 3
    assert torch.cuda.is_available(), "bench_wide_update.py needs a GPU"
    lines = []

    def emit(**rec):
        rec["wide_entry_points"] = HAS_WIDE
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        if args.out:      # written as it goes: a run cut short keeps its lines
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    (heads if args.mode == "heads" else learners)(args, emit)


if __name__ == "__main__":
    main()
