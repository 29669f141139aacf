#!/usr/bin/env python3
"""Generate tests/golden/tarmac_actor_cases.npz by RUNNING THE REFERENCE's TarMAC_Actor in the build container.

    python tests/golden/make_tarmac_golden.py

The reference is imported through oracle/ref_harness.py; nothing of it is copied.  The fixture is data only: for a handful of small
cases the float32 state_dict of a reference ``TarMAC_Actor``, observations [4, N, F] and the probabilities the reference module
computes in fp64 (a ``.double()`` copy of the same float32 weights: the fp64 truth for them).

Weights are torch's default init times 2, biases uniform in +-0.5, observations N(0, 1.5^2): with the default init alone the
probabilities sit at 0.33-0.67 and a wrong band would move them far less; scaled, they span 0.002-0.998.

Layout: ``names`` (the case names), and per case ``<name>/meta`` = int64 [F, N, c, hops, mode (0 neighbours, 1 none), with_comm, H, K, V],
``<name>/obs`` float32, ``<name>/probs`` float64 and ``<name>/sd/<state_dict key>`` float32.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "tarmac_actor_cases.npz")

from oracle import ref_harness  # noqa: E402

# name, F, N, c, hops, mode, with_comm, H, K, V.  One case at the reference's sizes (H = 64, K = 8, V = 16); the others keep the
# default K and V - or the other sizes the attention kernel is built for - on a narrow hidden state, so that the file stays small.
CASES = [
    ("f22_n20_c10", 22, 20, 10, 1, "neighbours", True, 64, 8, 16),
    ("f51_n50_c10_hops2", 51, 50, 10, 2, "neighbours", True, 8, 8, 16),
    ("f51_n5_c3", 51, 5, 3, 1, "neighbours", True, 8, 16, 32),
    ("f51_n2_c10", 51, 2, 10, 1, "neighbours", True, 8, 8, 16),
    ("f22_n6_c0", 22, 6, 0, 1, "neighbours", True, 8, 4, 4),
    ("f22_n20_none", 22, 20, 10, 1, "none", True, 8, 8, 16),
    ("f22_n20_nocomm", 22, 20, 10, 1, "neighbours", False, 8, 8, 16),
]


def main():
    import torch

    ref_harness.load_reference()
    from agents.network import TarMAC_Actor

    out = {"names": np.array([c[0] for c in CASES])}
    for i, (name, F, N, c, hops, mode, with_comm, H, K, V) in enumerate(CASES):
        torch.manual_seed(1000 + i)
        g = torch.Generator(device="cpu").manual_seed(2000 + i)
        actor = TarMAC_Actor(num_obs=F, num_key=K, num_value=V, hidden_state_size=H, num_action=2, number_agents_comm=c, comm_mode=mode,
                             device=torch.device("cpu"), comm_defect_prob=0, num_hops=hops, with_gru=False, with_comm=with_comm)
        with torch.no_grad():
            for pname, p in actor.named_parameters():
                if pname.endswith("weight"):
                    p.mul_(2.0)
                else:
                    p.uniform_(-0.5, 0.5, generator=g)
        obs = (torch.randn((4, N, F), generator=g) * 1.5).float()
        with torch.no_grad():
            probs = copy.deepcopy(actor).double()(obs.double())
        out[name + "/meta"] = np.array([F, N, c, hops, 1 if mode == "none" else 0, int(with_comm), H, K, V], dtype=np.int64)
        out[name + "/obs"] = obs.numpy()
        out[name + "/probs"] = probs.numpy().astype(np.float64)
        for key, w in actor.state_dict().items():
            out[name + "/sd/" + key] = w.detach().numpy().astype(np.float32)
        print("%-20s probabilities %.4f .. %.4f" % (name, probs.min().item(), probs.max().item()))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
