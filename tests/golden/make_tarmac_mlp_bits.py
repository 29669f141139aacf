#!/usr/bin/env python3
"""Generate tests/golden/tarmac_mlp_parent_bits.npz by RUNNING FusedTarMACActor.sample on the GPU at the commit whose bits are to be
pinned (the parent of a change that must not move them).

    python tests/golden/make_tarmac_mlp_bits.py

The existing suites hold the fused actor to the probability contract against fp64, which a reordered sum still passes.  This fixture
is the kernels' own output, bit for bit: ``action``, ``a_prob``, ``probs`` and the whole workspace - ``cat`` [A, H (+ V)], ``qkv``
[A, K + K + V], ``state`` [A, H] (hops > 1) - of one sample per case and precision.  tests/test_gpu_tarmac_mlp_bits.py reruns the
same cases and asks for ``np.array_equal`` on every array: same compiler, same flags, same MFMA sequence, same bits.

Inputs are CPU-seeded (the actors of tests/test_gpu_tarmac_fused.py: torch's default init with the weights doubled; N(0, 1) rows) at
(E, N) = (3, 23): 69 agents, a partial last tile for the 16-agent tiles of fp32 and the 32-agent tiles of bf16x3, tiles that span envs.

Layout: ``commit`` (the commit the library under test was built from: ``git rev-parse HEAD`` where the generator ran), ``names``, and
per name ``<name>/action`` uint8, ``<name>/a_prob``, ``<name>/probs``, ``<name>/cat``, ``<name>/qkv``,
``<name>/state`` float32 (arrays of a part the case does not have are empty).
"""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "tarmac_mlp_parent_bits.npz")

DEV = "cuda:0"
E, N = 3, 23
SEED, STEP = 5, 17
PRECISIONS = ("fp32", "bf16x3")
ARRAYS = ("action", "a_prob", "probs", "cat", "qkv", "state")
# name, F, H, K, V, hops, with_comm, greedy
CASES = [
    ("exact_hops1", 51, 64, 8, 16, 1, True, False),              # the exact forms
    ("exact_hops2", 51, 64, 8, 16, 2, True, False),              # ... and the exact rehop
    ("general_hops2", 64, 48, 16, 32, 2, True, False),           # the general forms, an odd block count
    ("unaligned_f3", 3, 64, 4, 4, 1, True, False),               # rows that are no whole float4s: vec0 = 0
    ("exact_nocomm", 51, 64, 8, 16, 1, False, False),
    ("exact_greedy", 51, 64, 8, 16, 1, True, True),
]


def run_case(case, index, precision):
    """One sample of the case -> {array name: numpy array}.  The workspace starts from zeros: every float of it is the kernels'."""
    import torch
    from mdr_amd.tarmac import FusedTarMACActor, TarMACActor

    _, F, H, K, V, hops, with_comm, greedy = case
    torch.manual_seed(11 + index)
    actor = TarMACActor(F, num_key=K, num_value=V, hidden_state_size=H, number_agents_comm=10, num_hops=hops, with_comm=with_comm)
    with torch.no_grad():
        for pname, p in actor.named_parameters():
            if pname.endswith("weight"):
                p.mul_(2.0)
    g = torch.Generator(device="cpu").manual_seed(1000 + index)
    obs = torch.randn((E, N, F), generator=g).to(DEV)
    fused = FusedTarMACActor.from_module(actor.to(DEV), precision=precision)
    A = E * N
    ws = fused.workspace(A, obs.device)
    ws.zero_()
    action, a_prob, probs = fused.sample(obs, SEED, STEP, greedy=greedy, want_probs=True)
    torch.cuda.synchronize()
    w = ws.cpu().numpy().view(np.float32)
    ldcat, ldqkv = (H + V if with_comm else H), K + K + V
    n_cat = A * ldcat
    n_qkv = A * ldqkv if with_comm else 0
    n_state = A * H if with_comm and hops > 1 else 0
    assert w.size >= n_cat + n_qkv + n_state
    return {"action": action.cpu().numpy(), "a_prob": a_prob.cpu().numpy(), "probs": probs.cpu().numpy(),
            "cat": w[:n_cat].reshape(A, ldcat).copy(), "qkv": w[n_cat:n_cat + n_qkv].reshape(-1, ldqkv).copy(),
            "state": w[n_cat + n_qkv:n_cat + n_qkv + n_state].reshape(-1, H).copy()}


def case_names():
    return ["%s/%s" % (c[0], p) for c in CASES for p in PRECISIONS]


def run(name):
    cname, precision = name.split("/")
    index = [c[0] for c in CASES].index(cname)
    return run_case(CASES[index], index, precision)


def main():
    head = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    out = {"commit": np.array(head), "names": np.array(case_names())}
    for name in case_names():
        got = run(name)
        for key in ARRAYS:
            out[name + "/" + key] = got[key]
        p = got["probs"]
        print("%-24s p0 %.4f .. %.4f, %d of %d actions are 1" % (name, p[:, 0].min(), p[:, 0].max(), int(got["action"].sum()), len(got["action"])))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
