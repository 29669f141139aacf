#!/usr/bin/env python3
"""Generate tests/golden/tarmac_a2c_cases.npz by RUNNING THE REFERENCE's MultiAgentPolicy (agents/tarmac/model.py) in the build container.

    python tests/golden/make_tarmac_a2c_golden.py

The reference is imported through oracle/ref_harness.py; nothing of it is copied.  The fixture is data only: for a few small cases the
float32 state_dict of a reference ``MultiAgentPolicy`` built as ``A2C_ACKTR.__init__`` builds it (recurrent_policy=False, one hop),
inputs, and what a ``.double()`` copy of the same module computes from them (the fp64 truth for these float32 weights): ``value``,
``logits``, ``x``, ``comm_out``, ``p_attn`` of ``act``'s forward; the three losses of ``update_multi_agent``'s formula
(agents/tarmac/a2c_acktr.py:81-96) through ``evaluate_actions``; the gradient of value_loss_coef value_loss + action_loss -
entropy_coef entropy for every parameter ``backward()`` reaches, and the names of those whose ``.grad`` stays None.

Weights are torch's default init times 2, biases uniform in +-0.5, ``dist.linear`` (orthogonal at gain 0.01) times 150 so that the
probabilities span well beyond 0.4-0.6, every parameter then rounded to a multiple of 2^-8 (the file has to stay below the largest
fixture here, and the fp64 gradients of the reference-size case alone take 320 KB); observations and messages N(0, 1), returns
N(0, 2^2).

Layout: ``names``; per case ``<name>/meta`` = int64 [N, F, C, S, K, B], ``<name>/coef`` = float64 [value_loss_coef, entropy_coef],
``<name>/obs``, ``<name>/comm_in``, ``<name>/returns`` float32, ``<name>/action`` int64, ``<name>/sd/<key>`` float32, the results
``<name>/value`` ... ``<name>/losses`` float64, ``<name>/grad/<key>`` float64 and ``<name>/no_grad`` (the names without a gradient).
"""
from __future__ import annotations

import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "tarmac_a2c_cases.npz")

from oracle import ref_harness  # noqa: E402

# name, N, F, C, S, K, B.  One case at the reference's sizes; the others are narrow so that the file stays small.
CASES = [
    ("n20_f22_reference", 20, 22, 32, 128, 16, 1),
    ("n1", 1, 22, 32, 16, 16, 3),
    ("n2", 2, 22, 32, 16, 16, 3),
    ("n5_s20_c8_k8", 5, 22, 8, 20, 8, 3),
    ("n50_s16", 50, 22, 32, 16, 16, 1),
]
VALUE_COEF, ENTROPY_COEF = 0.5, 0.01      # config_dict["TarMAC_prop"]
GRID = 256.0                              # every parameter is rounded to a multiple of 2^-8: the float32 arrays compress to half


def main():
    import torch

    ref_harness.load_reference()
    from agents.tarmac.model import CommAttention, MultiAgentPolicy

    out = {"names": np.array([c[0] for c in CASES])}
    for i, (name, N, F, C, S, K, B) in enumerate(CASES):
        torch.manual_seed(3000 + i)
        g = torch.Generator(device="cpu").manual_seed(4000 + i)
        policy = MultiAgentPolicy(n_agents=N, obs_size=F, num_actions=2, recurrent_policy=False, state_size=S, comm_size=C,
                                  comm_mode="from_states_rec_att", comm_num_hops=1, use_cnn=False, env="MA_DemandResponse")
        if K != 16:      # MultiAgentBase never passes key_size on
            policy.base.comm = CommAttention(state_size=S, comm_size=C, key_size=K, num_hops=1)
        with torch.no_grad():
            for pname, p in policy.named_parameters():
                if pname == "dist.linear.weight":
                    p.mul_(150.0)
                elif pname.endswith("weight"):
                    p.mul_(2.0)
                else:
                    p.uniform_(-0.5, 0.5, generator=g)
                p.copy_(torch.round(p * GRID) / GRID)
        obs = torch.randn((B, N, F), generator=g).float()
        comm_in = torch.randn((B, N, C), generator=g).float()
        returns = (torch.randn((B, N), generator=g) * 2).float()
        action = torch.randint(0, 2, (B, N), generator=g)
        dbl = copy.deepcopy(policy).double()
        states, masks = torch.zeros((B, N, S), dtype=torch.float64), torch.ones((B, 1), dtype=torch.float64)
        with torch.no_grad():
            value, x, _, comm_out, aux = dbl.base(obs.double(), states, comm_in.double(), masks)
            logits = dbl.dist.linear(x)
        full = aux["p_attn"][0]                                               # [(B N), (B N)]: the envs on the diagonal
        p_attn = torch.stack([full[b * N:(b + 1) * N, b * N:(b + 1) * N] for b in range(B)])
        assert float((full.sum() - p_attn.sum()).abs()) < 1e-12              # nothing outside the blocks
        values, logp, entropy, _ = dbl.evaluate_actions(obs.double(), states, comm_in.double(), masks, action.unsqueeze(-1))
        adv = returns.double().view(B, N, 1) - values.view(B, 1, 1).expand(B, N, 1)
        value_loss = adv.pow(2).mean()
        action_loss = -(adv.detach() * logp.view(B, N, 1)).mean()
        dbl.zero_grad()
        (value_loss * VALUE_COEF + action_loss - entropy * ENTROPY_COEF).backward()
        p = torch.softmax(logits, dim=-1)
        out[name + "/meta"] = np.array([N, F, C, S, K, B], dtype=np.int64)
        out[name + "/coef"] = np.array([VALUE_COEF, ENTROPY_COEF])
        out[name + "/obs"], out[name + "/comm_in"], out[name + "/returns"] = obs.numpy(), comm_in.numpy(), returns.numpy()
        out[name + "/action"] = action.numpy().astype(np.int64)
        for key, t in (("value", value.view(B)), ("logits", logits), ("x", x), ("comm_out", comm_out.view(B, N, C)), ("p_attn", p_attn),
                       ("losses", torch.stack([value_loss, action_loss, entropy]))):
            out[name + "/" + key] = t.detach().numpy().astype(np.float64)
        no_grad = []
        for key, q in dbl.named_parameters():
            if q.grad is None:
                no_grad.append(key)
            else:
                out[name + "/grad/" + key] = q.grad.numpy().astype(np.float64)
        out[name + "/no_grad"] = np.array(no_grad)
        for key, w in policy.state_dict().items():
            out[name + "/sd/" + key] = w.detach().numpy().astype(np.float32)
        print("%-20s probabilities %.4f .. %.4f, losses %s, %d tensors without a gradient" % (name, p.min().item(), p.max().item(),
                                                                                          out[name + "/losses"], len(no_grad)))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
