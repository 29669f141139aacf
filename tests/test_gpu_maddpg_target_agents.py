"""mdr_maddpg_target_agents (include/mdr_policy.h; csrc/mdr_maddpg_grad.hip, MODE_PICK_AGENTS) on the GPU against the fp64
restatement with per-agent picks and the derived bounds of tests/maddpg_agents_ref.py: next_action exactly, y and next_q at worst
|error| / bound <= 1.  Two exact oracles beside it: column k of next_action is what mdr_maddpg_target writes in column k with net k
as its shared target actor, and N equal nets give mdr_maddpg_target's bits on all three outputs."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import maddpg_agents_ref as A
from tests import maddpg_grad_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
CASES = [(net, B) for net in R.NETS[1:4] for B in (1, 15, 16, 17, 33)] + [(R.NETS[4], 33)]
MID = R.NETS[2]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class Call:
    """Both target calls on device copies of one case's inputs; outputs NaN / 0xEE-filled before each call."""

    def __init__(self, d, nets, agent, tau, index=None, noise=None):
        self.lib = nat.load()
        M, N, F = d["next_state"].shape
        self.N, self.agent, self.tau = N, agent, tau
        self.keep = [[_dev(net[k]) for k in R.PARAM_NAMES] for net in nets]
        Ha = nets[0]["W1"].shape[0]
        self.actors = (nat.MdrMlp * N)(*[nat.MdrMlp(C.sizeof(nat.MdrMlp), F, Ha, Ha, 2, *[_ptr(p) for p in params]) for params in self.keep])
        self.cparams = [_dev(d["tc" + k]) for k in R.PARAM_NAMES]
        Hc, J = d["tcW1"].shape
        self.critic = nat.MdrMlp(C.sizeof(nat.MdrMlp), J, Hc, Hc, 1, *[_ptr(p) for p in self.cparams])
        self.next_state, self.reward = _dev(d["next_state"]), _dev(d["reward"])
        self.index = index
        self.B = int(index.shape[0]) if index is not None else M
        self.noise = _dev(d["noise_t"] if noise is None else noise)
        self.ld = N * F

    def _outs(self):
        return (torch.full((self.B,), NAN, device=DEV), torch.full((self.B,), NAN, device=DEV),
                torch.full((self.B, self.N), 0xEE, dtype=torch.uint8, device=DEV))

    def agents(self, mw=0, **ov):
        y, nq, na = self._outs()
        a = dict(actors=self.actors, nets=self.N, critic=C.byref(self.critic), ns=_ptr(self.next_state), ld=self.ld, N=self.N, agent=self.agent,
                 noise=_ptr(self.noise), tau=self.tau, B=self.B)
        a.update(ov)
        rc = self.lib.mdr_maddpg_target_agents(a["actors"], a["nets"], a["critic"], a["ns"], a["ld"], _ptr(self.reward), _ptr(self.index), a["B"],
                                               a["N"], a["agent"], a["noise"], C.c_float(a["tau"]), C.c_float(R.GAMMA), mw, _ptr(y), _ptr(nq),
                                               _ptr(na), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        return rc, y, nq, na

    def shared(self, k, mw=0):
        y, nq, na = self._outs()
        rc = self.lib.mdr_maddpg_target(C.byref(self.actors[k]), C.byref(self.critic), _ptr(self.next_state), self.ld, _ptr(self.reward),
                                        _ptr(self.index), self.B, self.N, self.agent, _ptr(self.noise), C.c_float(self.tau), C.c_float(R.GAMMA),
                                        mw, _ptr(y), _ptr(nq), _ptr(na), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == nat.MDR_OK
        return y, nq, na


@pytest.mark.parametrize("tau", [1.0, 0.5])
@pytest.mark.parametrize("net,B", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_against_fp64_and_the_shared_kernel_column_by_column(net, B, tau):
    N = net[0]
    agent = N - 1
    case = A.reference(B, *net, agent, tau)
    call = Call(case["inputs"], case["nets"], agent, tau)
    rc, y, nq, na = call.agents()
    assert rc == nat.MDR_OK
    assert np.array_equal(na.cpu().numpy(), case["ref"]["next_action"])
    got = dict(y=y.cpu().numpy(), next_q=nq.cpu().numpy())
    for k in ("y", "next_q"):
        w = R.worst(got[k], case["ref"][k], case["bound"][k])
        print("TARGET_AGENTS %s B=%d tau=%.1f %s worst=%.4f" % (net, B, tau, k, w))
        assert w <= 1.0, (k, w)
    for k in range(N):
        assert torch.equal(call.shared(k)[2][:, k], na[:, k]), k


@pytest.mark.parametrize("B", [1, 17, 33])
def test_equal_nets_give_the_shared_kernels_bits(B):
    case = A.reference(B, *MID, 1, 1.0, equal=True)
    call = Call(case["inputs"], case["nets"], 1, 1.0)
    rc, y, nq, na = call.agents()
    ys, nqs, nas = call.shared(0)
    assert rc == nat.MDR_OK and torch.equal(na, nas)
    assert torch.equal(y.view(torch.int32), ys.view(torch.int32)) and torch.equal(nq.view(torch.int32), nqs.view(torch.int32))


def test_index_with_repeats_the_grid_and_two_calls():
    B = 16 * 3 + 5      # several tiles per agent and a partial one
    case = A.reference(R.PARENT_ROWS, *MID, 2, 1.0)
    d = case["inputs"]
    idx = np.random.default_rng(3).integers(0, R.PARENT_ROWS, B)
    idx[1] = idx[0]
    noise = np.ascontiguousarray(d["noise_t"][idx])      # per minibatch row: a repeated env-step keeps its pick
    call = Call(d, case["nets"], 2, 1.0, index=_dev(idx.astype(np.int64)), noise=noise)
    rc, y, nq, na = call.agents()
    assert rc == nat.MDR_OK
    gathered = {k: (np.ascontiguousarray(v[idx]) if k in R.ROW_KEYS else v) for k, v in d.items()}
    rc2, y2, nq2, na2 = Call(gathered, case["nets"], 2, 1.0).agents()
    assert rc2 == nat.MDR_OK
    for x, z in ((y, y2), (nq, nq2)):
        assert torch.equal(x.view(torch.int32), z.view(torch.int32))
    assert torch.equal(na, na2) and np.array_equal(na.cpu().numpy(), A.picks(gathered, case["nets"], 1.0))
    for mw in (2, 1):
        _, ym, nqm, nam = call.agents(mw=mw)
        assert torch.equal(ym.view(torch.int32), y.view(torch.int32)) and torch.equal(nqm.view(torch.int32), nq.view(torch.int32))
        assert torch.equal(nam, na)
    _, y3, nq3, na3 = call.agents()
    assert torch.equal(y3.view(torch.int32), y.view(torch.int32)) and torch.equal(nq3.view(torch.int32), nq.view(torch.int32)) and torch.equal(na3, na)


def test_refused_calls_write_nothing():
    case = A.reference(17, *MID, 0, 1.0)
    call = Call(case["inputs"], case["nets"], 0, 1.0)
    N = MID[0]
    other = Call(A.reference(17, *R.NETS[3], 0, 1.0)["inputs"], A.reference(17, *R.NETS[3], 0, 1.0)["nets"], 0, 1.0)
    mixed = (nat.MdrMlp * N)(call.actors[0], call.actors[1], call.actors[2])
    mixed[2].hidden1 = 96      # a differing shape
    bad_size = (nat.MdrMlp * N)(call.actors[0], call.actors[1], call.actors[2])
    bad_size[1].struct_size = 4
    many = (nat.MdrMlp * 33)(*[call.actors[0]] * 33)
    inv, uns = nat.MDR_ERR_INVALID, nat.MDR_ERR_UNSUPPORTED
    for ov, status in ((dict(actors=None), inv), (dict(nets=2), inv), (dict(nets=0), inv), (dict(N=2), inv), (dict(agent=N), inv),
                       (dict(agent=-1), inv), (dict(B=-1), inv), (dict(ld=N * MID[1] - 1), inv), (dict(tau=0.0), inv), (dict(noise=None), inv),
                       (dict(ns=None), inv), (dict(actors=bad_size), inv), (dict(actors=mixed), uns), (dict(actors=many, nets=33, N=33), uns)):
        rc, y, nq, na = call.agents(**ov)
        assert rc == status, ov
        assert bool(y.isnan().all()) and bool(nq.isnan().all()) and bool((na == 0xEE).all()), ov
    assert other.agents()[0] == nat.MDR_OK
    rc, y, nq, na = call.agents(B=0)
    assert rc == nat.MDR_OK and bool(y.isnan().all()) and bool((na == 0xEE).all())
