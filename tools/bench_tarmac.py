#!/usr/bin/env python3
"""TarMAC-PPO actor: mdr_tarmac_comm alone against its traffic floor and against the dense torch attention, its share of one full
TarMACActor.sample step, and - in the same run on the same device, on the same observations - the same step through FusedTarMACActor
in exact fp32 (csrc/mdr_tarmac_mlp.hip) and in bf16x3 (csrc/mdr_tarmac_mlp_bf16.hip) with the two floors of each of their kernels.  HIP
events after warm-up; one JSON line per measurement, the fused lines with their precision, and with both precisions how many actions
differ between the two fused forms and the largest difference of their a_prob.

    python tools/bench_tarmac.py [--shapes 4096x1024,83886x50] [--iters 50] [--warmup 5] [--hops 1] [--skip-attention]
                                 [--precision fp32|bf16x3|both] [--out FILE]

Per-kernel times of the fused step come from `rocprofv3 --kernel-trace --stats -- python tools/bench_tarmac.py --skip-attention`; the
floors to hold them against are the "floors" record: matrix time = the kernel's own count of v_mfma_f32_16x16x4_f32 per 16-agent tile x
15.0 ns per SIMD (tools/probe, mdr_policy.hip) over 1024 SIMDs, traffic = algorithmic bytes per agent at the rate below.  The bf16x3
kernels ("floors_bf16x3"): three v_mfma_f32_16x16x32_bf16 per (k-step, output block) pair and 16-agent column block at
MFMA_BF16_NS per SIMD - timed with tools/probe/mfma_issue_probe.hip (shape 16, no vector instructions in between, two waves per
SIMD: 4.856 ms for 2 x 20000 x 14 MFMAs per SIMD = 8.67 ns, profiles/tarmac_bf16_mfma_probe.txt) - the same bytes.

Floor: 4 (2 K + 2 V) algorithmic bytes per agent (query, key, value read once, comm written once: 192 B at K = 8, V = 16) over the
5.25 TB/s out-of-cache rate of DESIGN.md section 7.  The dense comparator is TarMAC_Comm.forward's formula (agents x agents scores,
masked softmax, attn @ value) on the same device: on all envs where its temporaries fit, else on the largest env count that does."""
import argparse
import ctypes as C
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mdr_amd  # noqa: E402
from mdr_amd.tarmac import FusedTarMACActor, TarMACActor  # noqa: E402

OUT_OF_CACHE_BPS = 5.25e12
K, V, COMM, F_OBS, HID = 8, 16, 10, 51, 64
MFMA_NS, MFMA_BF16_NS, SIMDS = 15.0, 8.67, 1024


def fused_floors(A, hops):
    """name -> (MFMAs per tile, algorithmic bytes per agent, matrix floor us, traffic floor us) for the kernels of one fused step."""
    nbh, nbv, nbm = (HID + 15) // 16, (V + 15) // 16, (HID + V + 15) // 16
    proj = 3 * 4 * nbh * nbh + 4 * nbh * (2 + nbv)
    kernels = {"k_tarmac_encode": ((F_OBS + 3) // 4 * nbh + 4 * nbh * nbh + proj, 4 * (F_OBS + HID + K + K + V)),
               "k_tarmac_head": ((HID + V) // 4 * nbh, 4 * (HID + V) + 1 + 4)}
    if hops > 1:
        kernels["k_tarmac_rehop"] = ((HID + V) // 4 * nbm + 4 * nbm * nbh + proj, 4 * (V + HID + HID + K + K + V))
    tiles = (A + 15) // 16
    return {n: dict(mfma_per_tile=m, bytes_per_agent=b, matrix_floor_us=round(m * MFMA_NS * 1e-3 * tiles / SIMDS, 1),
                    traffic_floor_us=round(A * b / OUT_OF_CACHE_BPS * 1e6, 1)) for n, (m, b) in kernels.items()}


def fused_floors_bf16(A, hops):
    """The same record for the bf16x3 kernels: MFMAs per 16-agent column block = 3 x the (k-step, output block) pairs."""
    nbh, nbv, nbm = (HID + 15) // 16, (V + 15) // 16, (HID + V + 15) // 16
    rows, regs = (lambda n: (n + 31) // 32), (lambda nbi: (nbi + 1) // 2)
    proj = regs(nbh) * (3 * nbh + 2 + nbv)
    kernels = {"k_tarmac_encode_bf16": (3 * ((rows(F_OBS) + regs(nbh)) * nbh + proj), 4 * (F_OBS + HID + K + K + V)),
               "k_tarmac_head_bf16": (3 * rows(HID + V) * nbh, 4 * (HID + V) + 1 + 4)}
    if hops > 1:
        kernels["k_tarmac_rehop_bf16"] = (3 * ((rows(V) + rows(HID)) * nbm + regs(nbm) * nbh + proj), 4 * (V + HID + HID + K + K + V))
    blocks = (A + 15) // 16
    return {n: dict(mfma_per_block=m, bytes_per_agent=b, matrix_floor_us=round(m * MFMA_BF16_NS * 1e-3 * blocks / SIMDS, 1),
                    traffic_floor_us=round(A * b / OUT_OF_CACHE_BPS * 1e6, 1)) for n, (m, b) in kernels.items()}


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
    ap.add_argument("--hops", type=int, default=1)
    ap.add_argument("--skip-attention", action="store_true", help="only the two full steps (the run to put under rocprofv3)")
    ap.add_argument("--precision", choices=("fp32", "bf16x3", "both"), default="both", help="the fused forms to measure")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_tarmac.py needs a GPU"
    lib = mdr_amd.load_native()
    lines = []

    def emit(**rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    for shape in args.shapes.split(","):
        E, N = (int(x) for x in shape.split("x"))
        A = E * N
        g = torch.Generator(device=DEV).manual_seed(1)
        qkv = torch.randn((A, K + K + V), device=DEV, generator=g)
        out = torch.empty((A, V), device=DEV)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def band():
            rc = lib.mdr_tarmac_comm(C.c_void_p(qkv.data_ptr()), K + K + V, C.c_void_p(qkv.data_ptr() + 4 * K), K + K + V,
                                     C.c_void_p(qkv.data_ptr() + 8 * K), K + K + V, E, N, K, V, COMM, 0, C.c_float(0.0), C.c_uint64(0),
                                     C.c_uint64(0), None, 0, C.c_void_p(out.data_ptr()), V, stream)
            assert rc == 0, rc

        us = None
        if not args.skip_attention:
            us = timed(band, args.iters, args.warmup)
            floor_us = A * 4 * (2 * K + 2 * V) / OUT_OF_CACHE_BPS * 1e6
            emit(what="mdr_tarmac_comm", envs=E, houses=N, agents=A, us=round(us, 2), floor_us=round(floor_us, 2), times_floor=round(us / floor_us, 3),
                 algorithmic_GBps=round(A * 4 * (2 * K + 2 * V) / us * 1e-3, 1))

            # dense torch attention on the same inputs: all envs if five [E, N, N] temporaries fit in half of the free memory
            free = torch.cuda.mem_get_info()[0]
            E_d = int(min(E, max(1, (free // 2) // (5 * 4 * N * N))))
            mask = TarMACActor(F_OBS).band_mask(N, DEV).float()
            qd, kd, vd = (t.reshape(E, N, -1)[:E_d].contiguous() for t in (qkv[:, :K], qkv[:, K:2 * K], qkv[:, 2 * K:]))
            us_dense = timed(lambda: dense_attention(qd, kd, vd, mask), max(3, args.iters // 10), 2)
            ref = dense_attention(qd, kd, vd, mask)
            err = float((ref - out.view(E, N, V)[:E_d]).abs().max())
            emit(what="dense torch attention", envs=E_d, houses=N, us=round(us_dense, 2), us_per_env=round(us_dense / E_d, 4),
                 band_us_per_env=round(us / E, 4), band_speedup_per_env=round((us_dense / E_d) / (us / E), 1), max_abs_diff_to_band=err)
            del qd, kd, vd, ref, mask

        # one full actor.sample step (GEMMs + attention + head); the attention's share sizes a later MLP fusion
        torch.manual_seed(0)
        actor = TarMACActor(F_OBS, num_hops=args.hops).to(DEV)
        obs = torch.randn((E, N, F_OBS), device=DEV, generator=g)
        action = torch.empty(A, dtype=torch.uint8, device=DEV)
        a_prob = torch.empty(A, dtype=torch.float32, device=DEV)
        us_step = timed(lambda: actor.sample(obs, 0, 0, action=action, a_prob=a_prob), max(3, args.iters // 5), 2)
        emit(what="TarMACActor.sample", envs=E, houses=N, hops=args.hops, us=round(us_step, 2),
             attention_share=round(us / us_step, 4) if us is not None else None, agent_steps_per_s=round(A / us_step * 1e6))
        # the same step as one chain of HIP kernels, per precision; the same-run eager time above is what it has to beat
        fused_out = {}
        for precision in (("fp32", "bf16x3") if args.precision == "both" else (args.precision,)):
            fused = FusedTarMACActor.from_module(actor, precision=precision)
            action_f, a_prob_f = torch.empty_like(action), torch.empty_like(a_prob)
            us_fused = timed(lambda: fused.sample(obs, 0, 0, action=action_f, a_prob=a_prob_f), max(3, args.iters // 5), 2)
            rec = dict(what="FusedTarMACActor.sample", precision=precision, envs=E, houses=N, hops=args.hops, us=round(us_fused, 2),
                       eager_us=round(us_step, 2), speedup=round(us_step / us_fused, 2), agent_steps_per_s=round(A / us_fused * 1e6),
                       actions_differ_from_eager=int((action != action_f).sum()),
                       max_abs_a_prob_diff_to_eager=float((a_prob - a_prob_f).abs().max()))
            if "fp32" in fused_out:      # bf16x3 against the fused fp32 form of this run: same observations, same draws
                a32, p32, us32 = fused_out["fp32"]
                rec.update(fp32_us=round(us32, 2), speedup_over_fp32=round(us32 / us_fused, 2), actions_differ=int((a32 != action_f).sum()),
                           max_abs_a_prob_diff=float((p32 - a_prob_f).abs().max()))
            else:
                rec.update(actions_differ=rec["actions_differ_from_eager"], max_abs_a_prob_diff=rec["max_abs_a_prob_diff_to_eager"])
            emit(**rec)
            fused_out[precision] = (action_f, a_prob_f, us_fused)
            del fused
        if "fp32" in fused_out:
            emit(what="floors", envs=E, houses=N, hops=args.hops, **fused_floors(A, args.hops))
        if "bf16x3" in fused_out:
            emit(what="floors_bf16x3", envs=E, houses=N, hops=args.hops, mfma_ns=MFMA_BF16_NS,
                 **fused_floors_bf16(A, args.hops))
        del actor, fused_out, obs, qkv, out
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
