#!/usr/bin/env python3
"""The comm modes "all" and "random_sample" of the TarMAC-PPO actor: mdr_tarmac_gather and the whole actor with ``attention="gather"``
against the only way the parent had to evaluate these masks - the dense torch formula (``TarMACActor.dense_logits`` with the same
masks) on the same device.  HIP events after warm-up; the two arms alternate inside one process, every figure is the median of
``--repeats`` windows with their minimum and maximum beside it; one JSON line per measurement.

    python tools/bench_tarmac_gather.py [--shapes 4096x1024,83886x50] [--train-shape 256x20] [--iters 20] [--repeats 7] [--out FILE]

Measured per shape and mode: the attention alone (kernel vs the dense masked softmax on the packed projections), one whole actor step
(``sample``), and at ``--train-shape`` - the reference's minibatch - forward(differentiable=True) + backward of a scalar loss.  The
dense arm materialises [E, N, N] tensors, so it runs on the first E_d envs whose temporaries fit and is compared per env.  The masks of
"random_sample" are the restated draw of tests/tarmac_gather_ref.py for the same key, so both arms compute the same thing; the largest
difference between them is reported.

Per-kernel times come from ``rocprofv3 --kernel-trace --stats -- python tools/bench_tarmac_gather.py --skip-dense`` in a run of its own."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mdr_amd  # noqa: E402
from mdr_amd.tarmac import GATHER_MODES, TarMACActor  # noqa: E402
from tests import tarmac_gather_ref as gr  # noqa: E402

K, V, COMM, F_OBS = 8, 16, 10, 51
DEV = "cuda:0"
SEED, STEP = 7, 3


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def alternate(arms, iters, repeats, warmup=3):
    """{name: fn} -> {name: (median, min, max) us}: every arm warmed up, then `repeats` rounds of one window per arm in turn."""
    for fn in arms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n in arms}
    for _ in range(repeats):
        for n, fn in arms.items():
            times[n].append(window(fn, iters))
    return {n: (statistics.median(t), min(t), max(t)) for n, t in times.items()}


def stats(prefix, t, per=1):
    return {prefix + "_us": round(t[0] / per, 4), prefix + "_min_us": round(t[1] / per, 4), prefix + "_max_us": round(t[2] / per, 4)}


def dense_attention(q, k, v, mask):
    s = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(q.shape[-1])
    s = s - s.max(dim=-1, keepdim=True)[0]
    e = torch.exp(s) * mask
    a = e / e.sum(dim=-1, keepdim=True)
    return torch.matmul(torch.where(torch.isnan(a), torch.zeros_like(a), a), v)


def masks_for(mode, E, N, hops=1):
    """bool [hops, E, N, N] ("all": [hops, N, N] ones) on the device: what the kernels draw for (SEED, STEP)."""
    if mode == "all":
        return torch.ones((hops, N, N), dtype=torch.bool, device=DEV)
    return torch.from_numpy(np.stack([gr.mask_of(gr.sample_index(E, N, COMM, SEED, STEP, 0, h), N) for h in range(hops)])).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x1024,83886x50")
    ap.add_argument("--train-shape", default="256x20")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--skip-dense", action="store_true", help="the kernels and the gather actor only (the run to put under rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tarmac_gather.py needs a GPU"
    lib = mdr_amd.load_native()
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def shape_of(text):
        return tuple(int(x) for x in text.split("x"))

    for E, N in [shape_of(s) for s in args.shapes.split(",") if s]:
        A = E * N
        E_d = int(min(E, max(1, 2 ** 28 // (N * N))))      # the dense arm's [E_d, N, N] float tensors: at most 1 GiB each
        gen = torch.Generator(device=DEV).manual_seed(1)
        ld = K + K + V
        qkv = torch.randn((A, ld), device=DEV, generator=gen)
        out = torch.empty((A, V), device=DEV)
        obs = torch.randn((E, N, F_OBS), device=DEV, generator=gen)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = qkv.data_ptr()
        for mode in ("all", "random_sample"):
            def kernel():
                rc = lib.mdr_tarmac_gather(C.c_void_p(p), ld, C.c_void_p(p + 4 * K), ld, C.c_void_p(p + 8 * K), ld, E, N, K, V, COMM,
                                           GATHER_MODES[mode], C.c_uint64(SEED), C.c_uint64(STEP), None, 0, C.c_void_p(out.data_ptr()), V, stream)
                assert rc == 0, rc

            torch.manual_seed(0)
            actor = TarMACActor(F_OBS, comm_mode=mode, attention="gather").to(DEV)
            arms = {"kernel": kernel, "actor": lambda: actor.sample(obs, SEED, STEP)}
            diff = {}
            if not args.skip_dense:
                mask = masks_for(mode, E_d, N)
                qd, kd, vd = (qkv.view(E, N, ld)[:E_d, :, a:b].contiguous() for a, b in ((0, K), (K, 2 * K), (2 * K, ld)))
                fmask = mask[0].float()
                dense = copy_actor(actor)
                obs_d = obs[:E_d].contiguous()
                arms["dense_attention"] = lambda: dense_attention(qd, kd, vd, fmask)
                arms["dense_actor"] = lambda: dense.sample(obs_d, SEED, STEP, mask=mask)
                kernel()
                diff["attention_max_abs_diff"] = float((dense_attention(qd, kd, vd, fmask) - out.view(E, N, V)[:E_d]).abs().max())
                diff["actor_max_abs_diff"] = float((dense.sample(obs_d, SEED, STEP, mask=mask, want_probs=True)[2] -
                                                    actor.sample(obs_d, SEED, STEP, want_probs=True)[2]).abs().max())
            t = alternate(arms, args.iters, args.repeats)
            rec = dict(what="attention + actor step (sample)", mode=mode, envs=E, houses=N, agents=A, **stats("kernel", t["kernel"]),
                       **stats("actor", t["actor"]), attention_share_of_actor=round(t["kernel"][0] / t["actor"][0], 4))
            if not args.skip_dense:
                rec.update(dense_envs=E_d, **stats("kernel_per_env", t["kernel"], E), **stats("dense_attention_per_env", t["dense_attention"], E_d),
                           **stats("actor_per_env", t["actor"], E), **stats("dense_actor_per_env", t["dense_actor"], E_d),
                           attention_speedup_per_env=round((t["dense_attention"][0] / E_d) / (t["kernel"][0] / E), 2),
                           actor_speedup_per_env=round((t["dense_actor"][0] / E_d) / (t["actor"][0] / E), 2), **diff)
            emit(**rec)
            del actor
        del qkv, out, obs
        torch.cuda.empty_cache()

    # the training evaluation at the reference's minibatch: forward(differentiable=True) and the backward of a scalar loss
    E, N = shape_of(args.train_shape)
    gen = torch.Generator(device=DEV).manual_seed(2)
    obs = torch.randn((E, N, F_OBS), device=DEV, generator=gen)
    W = torch.randn((E, N, 2), device=DEV, generator=gen)
    for mode in ("all", "random_sample"):
        torch.manual_seed(0)
        actor = TarMACActor(F_OBS, comm_mode=mode, attention="gather").to(DEV)

        def step(a=actor, **kw):
            a.zero_grad(set_to_none=True)
            (a(obs, seed=SEED, step=STEP, **kw) * W).sum().backward()

        arms = {"gather": lambda: step(differentiable=True)}
        if not args.skip_dense:
            mask = masks_for(mode, E, N)
            dense = copy_actor(actor)
            arms["dense"] = lambda: step(dense, mask=mask)
        t = alternate(arms, args.iters, args.repeats)
        rec = dict(what="forward(differentiable=True) + backward", mode=mode, envs=E, houses=N, **stats("gather", t["gather"]))
        if not args.skip_dense:
            step(differentiable=True)
            g_gather = [p.grad.clone() for p in actor.parameters() if p.grad is not None]
            step(dense, mask=mask)
            g_dense = [p.grad for p in dense.parameters() if p.grad is not None]
            # per tensor ||gather - dense|| / ||dense||; a gradient that vanishes exactly (hidden2key's last bias: below 1e-6 of the
            # largest norm) is taken relative to that largest norm
            top = max(float(b.norm()) for b in g_dense)
            rec.update(**stats("dense", t["dense"]), gather_speedup=round(t["dense"][0] / t["gather"][0], 2),
                       grad_max_rel_l2_diff=max(float((a - b).norm()) / (float(b.norm()) if float(b.norm()) > 1e-6 * top else top)
                                                for a, b in zip(g_gather, g_dense)))
        emit(**rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def copy_actor(actor):
    """The same weights evaluated by the dense torch formula."""
    import copy
    dense = copy.deepcopy(actor)
    dense.attention = "dense"
    return dense


if __name__ == "__main__":
    main()
