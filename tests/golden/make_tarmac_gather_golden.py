#!/usr/bin/env python3
"""Generate tests/golden/tarmac_gather_cases.npz by RUNNING THE REFERENCE's TarMAC_Actor in the comm modes "all" and "random_sample".

    python tests/golden/make_tarmac_gather_golden.py

As tests/golden/make_tarmac_golden.py: the reference is imported through oracle/ref_harness.py, nothing of it is copied; weights are
torch's default init times 2, biases uniform in +-0.5, observations N(0, 1.5^2); the probabilities are those of a ``.double()`` copy
of the same float32 weights.  For "random_sample" the masks the reference's ``make_masks`` returned during that forward - one per hop,
drawn with np.random, shared by the batch - are recorded too: data, replayed through ``TarMACActor.forward(mask=)``.  For "all" the
recorded masks are the ones it returned as well (ones).

Layout: ``names``, and per case ``<name>/meta`` = int64 [F, N, c, hops, mode (0 all, 1 random_sample), H, K, V], ``<name>/obs`` float32
[4, N, F], ``<name>/probs`` float64 [4, N, 2], ``<name>/masks`` uint8 [hops, N, N] and ``<name>/sd/<state_dict key>`` float32.
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "tarmac_gather_cases.npz")

from oracle import ref_harness  # noqa: E402

# name, F, N, c, hops, mode, H, K, V.  One case at the reference's hidden size, the others at H = 8 so that the file stays small.
CASES = [
    ("all_n20", 22, 20, 10, 1, "all", 64, 8, 16),
    ("all_n50_hops2", 51, 50, 10, 2, "all", 8, 8, 16),
    ("random_n20_c10", 22, 20, 10, 1, "random_sample", 8, 8, 16),
    ("random_n5_c3_hops2", 51, 5, 3, 2, "random_sample", 8, 16, 32),
]


def main():
    import torch

    ref_harness.load_reference()
    from agents.network import TarMAC_Actor

    out = {"names": np.array([c[0] for c in CASES])}
    for i, (name, F, N, c, hops, mode, H, K, V) in enumerate(CASES):
        torch.manual_seed(3000 + i)
        np.random.seed(4000 + i)
        g = torch.Generator(device="cpu").manual_seed(5000 + i)
        actor = TarMAC_Actor(num_obs=F, num_key=K, num_value=V, hidden_state_size=H, num_action=2, number_agents_comm=c, comm_mode=mode,
                             device=torch.device("cpu"), comm_defect_prob=0, num_hops=hops, with_gru=False, with_comm=True)
        with torch.no_grad():
            for pname, p in actor.named_parameters():
                if pname.endswith("weight"):
                    p.mul_(2.0)
                else:
                    p.uniform_(-0.5, 0.5, generator=g)
        obs = (torch.randn((4, N, F), generator=g) * 1.5).float()
        twin = copy.deepcopy(actor).double()
        masks = []
        make_masks = twin.comm.make_masks

        def recording(number_agents):
            mask = make_masks(number_agents)
            masks.append(mask.detach().cpu().numpy() != 0)
            return mask

        twin.comm.make_masks = recording
        with torch.no_grad():
            probs = twin(obs.double())
        assert len(masks) == hops
        out[name + "/meta"] = np.array([F, N, c, hops, 0 if mode == "all" else 1, H, K, V], dtype=np.int64)
        out[name + "/obs"] = obs.numpy()
        out[name + "/probs"] = probs.numpy().astype(np.float64)
        out[name + "/masks"] = np.stack(masks).astype(np.uint8)
        for key, w in actor.state_dict().items():
            out[name + "/sd/" + key] = w.detach().numpy().astype(np.float32)
        print("%-20s probabilities %.4f .. %.4f, senders per receiver %s" % (name, probs.min().item(), probs.max().item(),
                                                                             sorted(set(np.stack(masks).sum(axis=2).ravel().tolist()))))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
