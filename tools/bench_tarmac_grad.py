#!/usr/bin/env python3
"""Backward of the banded TarMAC attention: mdr_tarmac_comm_backward against its traffic floor and against torch autograd of the
dense formula on the same device, and one TarMACActor.forward(differentiable=True) + backward step.  HIP events after warm-up; one
JSON line per measurement.

    python tools/bench_tarmac_grad.py [--shapes 4096x1024,83886x50] [--iters 50] [--warmup 5] [--skip-dense] [--out FILE]

Per-kernel times come from `rocprofv3 --kernel-trace --stats -- python tools/bench_tarmac_grad.py --skip-dense` in a run of its own
(k_tarmac_grad_recv, k_tarmac_grad_send).

Floor: query, key, value, out and grad_out read once, the three gradients written once - 4 (4 K + 4 V) = 384 algorithmic bytes per
agent at K = 8, V = 16 - plus the workspace's 16 bytes written and 16 read, over the 5.25 TB/s out-of-cache rate of DESIGN.md
section 7.  As launched, the sender-major kernel reads query, grad_out, key and value a second time (192 bytes more per agent, not
in the floor).  The dense comparator is the backward of TarMAC_Comm.forward's formula (agents x agents scores, masked softmax,
attn @ value) through torch autograd on a retained graph, on the largest env count whose temporaries fit."""
import argparse
import ctypes as C
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mdr_amd  # noqa: E402
from mdr_amd.tarmac import TarMACActor  # noqa: E402

OUT_OF_CACHE_BPS = 5.25e12
K, V, COMM, F_OBS = 8, 16, 10, 51
DEV = "cuda:0"


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3      # us


def dense_attention(q, k, v, mask):
    s = torch.matmul(q, k.transpose(-2, -1)) / math.sqrt(q.shape[-1])
    s = s - s.max(dim=-1, keepdim=True)[0]
    e = torch.exp(s) * mask
    a = e / e.sum(dim=-1, keepdim=True)
    return torch.matmul(torch.where(torch.isnan(a), torch.zeros_like(a), a), v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x1024,83886x50")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--skip-dense", action="store_true", help="the kernels and the actor step only (the run to put under rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tarmac_grad.py needs a GPU"
    lib = mdr_amd.load_native()
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for shape in args.shapes.split(","):
        E, N = (int(x) for x in shape.split("x"))
        A = E * N
        gen = torch.Generator(device=DEV).manual_seed(1)
        ld = K + K + V
        qkv = torch.randn((A, ld), device=DEV, generator=gen)
        g = torch.randn((A, V), device=DEV, generator=gen)
        out = torch.empty((A, V), device=DEV)
        grads = torch.empty((A, ld), device=DEV)      # dq | dk | dv packed as the operands are
        ws = torch.empty(lib.mdr_tarmac_comm_backward_workspace_bytes(A, K, V), dtype=torch.uint8, device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = qkv.data_ptr()
        operands = (C.c_void_p(p), ld, C.c_void_p(p + 4 * K), ld, C.c_void_p(p + 8 * K), ld, E, N, K, V, COMM, 0, C.c_float(0.0), C.c_uint64(0),
                    C.c_uint64(0), None, 0)

        def forward():
            rc = lib.mdr_tarmac_comm(*operands, C.c_void_p(out.data_ptr()), V, stream)
            assert rc == 0, rc

        def backward():
            d = grads.data_ptr()
            rc = lib.mdr_tarmac_comm_backward(*operands, C.c_void_p(out.data_ptr()), V, C.c_void_p(g.data_ptr()), V, C.c_void_p(d), ld,
                                              C.c_void_p(d + 4 * K), ld, C.c_void_p(d + 8 * K), ld, C.c_void_p(ws.data_ptr()), stream)
            assert rc == 0, rc

        us_fwd = timed(forward, args.iters, args.warmup)
        us = timed(backward, args.iters, args.warmup)
        floor_bytes = 4 * (4 * K + 4 * V) + 32
        floor_us = A * floor_bytes / OUT_OF_CACHE_BPS * 1e6
        emit(what="mdr_tarmac_comm_backward", envs=E, houses=N, agents=A, us=round(us, 2), forward_us=round(us_fwd, 2),
             floor_bytes_per_agent=floor_bytes, floor_us=round(floor_us, 2), times_floor=round(us / floor_us, 3),
             algorithmic_GBps=round(A * floor_bytes / us * 1e-3, 1))

        if not args.skip_dense:
            # autograd of the dense formula: about ten [E, N, N] tensors saved or temporary
            free = torch.cuda.mem_get_info()[0]
            E_d = int(min(E, max(1, (free // 2) // (10 * 4 * N * N))))
            mask = TarMACActor(F_OBS).band_mask(N, DEV).float()
            qd, kd, vd = (t.reshape(E, N, -1)[:E_d].contiguous().requires_grad_() for t in (qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:]))
            gd = g.view(E, N, V)[:E_d].contiguous()
            od = dense_attention(qd, kd, vd, mask)
            us_dense = timed(lambda: torch.autograd.grad(od, (qd, kd, vd), gd, retain_graph=True), max(3, args.iters // 10), 2)
            ref = torch.autograd.grad(od, (qd, kd, vd), gd)
            err = [float((r - grads.view(E, N, ld)[:E_d, :, a:b]).abs().max()) for r, (a, b) in zip(ref, ((0, K), (K, 2 * K), (2 * K, ld)))]
            emit(what="dense torch autograd backward", envs=E_d, houses=N, us=round(us_dense, 2), us_per_env=round(us_dense / E_d, 4),
                 band_us_per_env=round(us / E, 4), band_speedup_per_env=round((us_dense / E_d) / (us / E), 1), max_abs_diff_to_band=err)
            del qd, kd, vd, gd, od, ref, mask

        # one training evaluation of the whole actor: forward(differentiable=True) and the backward of a scalar loss
        torch.manual_seed(0)
        actor = TarMACActor(F_OBS).to(DEV)
        obs = torch.randn((E, N, F_OBS), device=DEV, generator=gen)
        W = torch.randn((E, N, 2), device=DEV, generator=gen)

        def step():
            actor.zero_grad(set_to_none=True)
            (actor(obs, differentiable=True) * W).sum().backward()

        us_step = timed(step, max(3, args.iters // 5), 2)
        emit(what="TarMACActor forward(differentiable=True) + backward", envs=E, houses=N, us=round(us_step, 2),
             attention_backward_share=round(us / us_step, 4), attention_forward_share=round(us_fwd / us_step, 4))
        del actor, obs, W, qkv, g, out, grads, ws
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
