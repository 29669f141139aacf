"""mdr_tarmac_critic_value / mdr_tarmac_critic_grad (include/mdr_policy.h) and mdr_amd.tarmac_ppo's critic calls on the GPU, against the
fp64 restatement and the derived rounding bound of tests/tarmac_critic_ref.py: every element of every output at worst |error| /
bound <= 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import tarmac_critic_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
OUTS = ("grad", "loss", "value", "advantage")
MID = (3, 51, 64)      # four tiles per workgroup


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Call:
    """The two C calls on device copies of a case's inputs; every output and the workspace NaN-filled before each."""

    def __init__(self, d, max_workgroups=0, index=None, state=None, ld=None, pad=0):
        self.lib = nat.load()
        self.mw = max_workgroups
        M, N, F = d["state"].shape
        self.N, self.F, self.J = N, F, N * F
        self.params = [_dev(d[k]) for k in R.PARAM_NAMES]
        H = d["W1"].shape[0]
        self.net = nat.MdrMlp(C.sizeof(nat.MdrMlp), N * F, H, d["W2"].shape[0], N, *[_ptr(p) for p in self.params])
        self.state = _dev(d["state"]) if state is None else state
        self.ld = N * F if ld is None else ld
        self.target = _dev(d["target"])
        self.index = index
        self.B = int(index.shape[0]) if index is not None else M
        self.G = int(self.lib.mdr_tarmac_critic_grad_floats(C.byref(self.net)))
        nbytes = int(self.lib.mdr_tarmac_critic_workspace_bytes(C.byref(self.net), self.B, max_workgroups))
        assert self.G > 0 and nbytes > 0
        self.pad = pad      # canary elements on either side of every output
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        sizes = (("grad", self.G), ("loss", 1), ("value", self.B * N), ("advantage", self.B * N), ("value_only", self.B * N))
        self.bufs = {k: torch.empty(n + 2 * pad, dtype=torch.float32, device=DEV) for k, n in sizes}

    def out(self, k):
        b = self.bufs[k]
        return b[self.pad:b.numel() - self.pad]

    def run_grad(self, **ov):
        self.ws.fill_(NAN)
        for k in OUTS:
            self.bufs[k].fill_(NAN)
        a = dict(critic=C.byref(self.net), state=_ptr(self.state), ld=self.ld, target=_ptr(self.target), index=_ptr(self.index), B=self.B,
                 mw=self.mw, ws=_ptr(self.ws), grad=_ptr(self.out("grad")), loss=_ptr(self.out("loss")), value=_ptr(self.out("value")),
                 advantage=_ptr(self.out("advantage")))
        a.update(ov)
        return self.lib.mdr_tarmac_critic_grad(a["critic"], a["state"], a["ld"], a["target"], a["index"], a["B"], a["mw"], a["ws"], a["grad"],
                                               a["loss"], a["value"], a["advantage"], _stream())

    def run_value(self, **ov):
        self.bufs["value_only"].fill_(NAN)
        a = dict(critic=C.byref(self.net), state=_ptr(self.state), ld=self.ld, index=_ptr(self.index), B=self.B, mw=self.mw,
                 value=_ptr(self.out("value_only")))
        a.update(ov)
        return self.lib.mdr_tarmac_critic_value(a["critic"], a["state"], a["ld"], a["index"], a["B"], a["mw"], a["value"], _stream())

    def results(self):
        r = {k: self.out(k).cpu().numpy() for k in ("grad", "value_only")}
        for k in ("value", "advantage"):
            r[k] = self.out(k).cpu().numpy().reshape(self.B, self.N)
        r["value_only"] = r["value_only"].reshape(self.B, self.N)
        r["loss"] = self.out("loss").cpu().numpy()[0]
        # dV [Bp][pad16(N)] sits behind h1, dz1, h2, dz2 in the workspace
        Bp = (self.B + 15) // 16 * 16
        H1p, H2p, Np = ((int(n) + 15) // 16 * 16 for n in (self.net.hidden1, self.net.hidden2, self.N))
        off = Bp * (2 * H1p + 2 * H2p)
        ws = self.ws.cpu().numpy()
        r["dV_padded"] = ws[off:off + Bp * Np].reshape(Bp, Np)
        r["dV"] = r["dV_padded"][:self.B, :self.N]
        return r

    def untouched(self, keys):
        return all(bool(torch.isnan(self.bufs[k]).all()) for k in keys)

    def canaries_intact(self):
        p = self.pad
        return all(bool(torch.isnan(torch.cat([b[:p], b[b.numel() - p:]])).all()) for b in self.bufs.values())


WORST = {}


def _check(got, r, label):
    for k in R.FLOAT_KEYS:
        w = R.worst(got[k], r["ref"][k], r["bound"][k])
        WORST[k] = max(WORST.get(k, 0.0), w)
        print("%s %-9s worst |error| / bound = %.3f" % (label, k, w))
        assert np.isfinite(np.asarray(got[k])).all(), (label, k)
        assert w <= 1.0, (label, k, w)


def _bits_equal(ra, rb, keys=("grad", "loss", "value", "advantage", "dV")):
    for k in keys:
        assert np.array_equal(np.asarray(ra[k]).view(np.uint32), np.asarray(rb[k]).view(np.uint32)), k


SWEEP = [(B,) + net for net in R.NETS for B in R.ROWS]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "B%d-N%d-F%d-H%d" % c)
def test_sweep_matches_fp64_within_the_bound(case, record_property):
    r = R.reference(*case)
    call = Call(r["inputs"])
    assert call.run_grad() == nat.MDR_OK and call.run_value() == nat.MDR_OK
    got = call.results()
    _check(got, r, "B%d N%d F%d H%d" % case)
    assert np.array_equal(got["value_only"].view(np.uint32), got["value"].view(np.uint32))      # the forward alone: the same bits
    # rows and agents past the batch carry zero dV
    assert not got["dV_padded"][case[0]:].any() and not got["dV_padded"][:, case[1]:].any()
    record_property("worst_ratio", max(WORST.values()))
    print("worst |error| / bound so far: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def _case(d, index=None):
    return dict(inputs=d, ref=R.evaluate(d, index=index), bound=R.bound(d, index=index))


@pytest.mark.parametrize("net,B,mw", [(MID, 63, 2), (MID, 64, 2), (MID, 65, 2), (MID, 129, 2), (MID, 65, 1), (R.NETS[5], 129, 2),
                                      (R.NETS[3], 16 * 7 + 5, 2), (R.NETS[1], 16 * 17 + 1, 2), (R.NETS[4], 16 * 11, 2)], ids=str)
def test_few_workgroups_give_the_bits_of_the_default_grid(net, B, mw):
    """max_workgroups = 2 (or 1): several tiles per workgroup, a partial tile, one row beyond a whole pass of the multi-tile grid (at
    64 hidden units a workgroup takes 4 tiles: 64 rows, two take 128); the weight pass loops over its blocks as well."""
    r = _case(R.inputs(B, *net))
    a, b = Call(r["inputs"], max_workgroups=mw), Call(r["inputs"])
    assert a.run_grad() == nat.MDR_OK and b.run_grad() == nat.MDR_OK and a.run_value() == nat.MDR_OK
    ra, rb = a.results(), b.results()
    _bits_equal(ra, rb)
    assert np.array_equal(ra["value_only"].view(np.uint32), rb["value"].view(np.uint32))
    _check(ra, r, "N%d F%d H%d B%d max_workgroups=%d" % (net + (B, mw)))


def test_one_tile_beyond_a_full_pass_of_the_library_grid():
    """The library's own grid loops: cap workgroups of 4 tiles each and one tile more (one row of it); the bits of a grid of two."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 16 * 4 * min(cus, 512) + 1
    assert B < 10 ** 5
    d = R.inputs(B, *MID)
    a, b = Call(d), Call(d, max_workgroups=2)
    assert a.run_grad() == nat.MDR_OK and b.run_grad() == nat.MDR_OK and a.run_value() == nat.MDR_OK
    ra, rb = a.results(), b.results()
    _bits_equal(ra, rb)
    assert np.array_equal(ra["value_only"].view(np.uint32), ra["value"].view(np.uint32))
    ref = R.evaluate(d)
    bnd = R.bound(d)
    _check(ra, dict(ref=ref, bound=bnd), "B%d own grid" % B)


def test_index_equals_the_gathered_copy_bit_for_bit():
    M, B = 65, 40
    d = R.inputs(M, *MID)
    idx = np.random.default_rng(5).integers(0, M, B)
    idx[:4] = [60, 3, 60, 3]      # repeats, out of order
    gathered = dict(d, state=d["state"][idx], target=d["target"][idx])
    a, b = Call(d, index=_dev(idx.astype(np.int64))), Call(gathered)
    assert a.run_grad() == nat.MDR_OK and b.run_grad() == nat.MDR_OK and a.run_value() == nat.MDR_OK and b.run_value() == nat.MDR_OK
    ra, rb = a.results(), b.results()
    _bits_equal(ra, rb, ("grad", "loss", "value", "advantage", "dV", "value_only"))
    _check(ra, _case(d, index=idx), "index")


def test_strided_env_steps_and_canaries():
    B, (N, F, H) = 33, R.NETS[3]
    r = R.reference(B, N, F, H)
    J = N * F
    wide = torch.full((B, J + 29), NAN, dtype=torch.float32, device=DEV)
    wide[:, 7:7 + J] = _dev(r["inputs"]["state"]).reshape(B, -1)
    call = Call(r["inputs"], state=wide[:, 7:7 + J], ld=J + 29, pad=64)
    assert call.run_grad() == nat.MDR_OK and call.run_value() == nat.MDR_OK
    assert call.canaries_intact()
    got = call.results()
    _check(got, r, "ld_state=%d" % (J + 29))
    assert np.array_equal(got["value_only"].view(np.uint32), got["value"].view(np.uint32))


def test_two_calls_give_equal_bits():
    r = R.reference(65, *R.NETS[5])
    call = Call(r["inputs"], max_workgroups=3)
    assert call.run_grad() == nat.MDR_OK
    first = call.results()
    assert call.run_grad() == nat.MDR_OK
    _bits_equal(first, call.results())


def test_nan_in_target_reaches_loss_and_advantage_and_stays_out_of_value():
    d = R.inputs(33, *MID)
    call = Call(d)
    call.target[17, 1] = NAN
    assert call.run_grad() == nat.MDR_OK
    got = call.results()
    s = R.param_slices(3 * 51, 64, 64, 3)
    assert np.isnan(got["loss"]) and np.isnan(got["grad"][s["b3"]][1]) and not np.isnan(got["grad"][s["b3"]][[0, 2]]).any()
    assert np.isnan(got["advantage"]).sum() == 1 and np.isnan(got["advantage"][17, 1])
    assert np.isnan(got["value"]).sum() == 0


def test_zero_rows_write_zeros():
    call = Call(R.inputs(16, *MID))
    assert call.run_value(B=0) == nat.MDR_OK and call.untouched(("value_only",))
    assert call.run_grad(B=0) == nat.MDR_OK
    assert bool((call.out("grad") == 0).all()) and float(call.out("loss")[0]) == 0.0 and call.untouched(("value", "advantage"))


def _wrong(net, **fields):
    twin = nat.MdrMlp.from_buffer_copy(net)
    for k, v in fields.items():
        setattr(twin, k, v)
    return C.byref(twin)


def test_refusals_leave_every_output_untouched():
    call = Call(R.inputs(33, *MID))
    J = call.J
    short = call.net.struct_size - 8
    invalid = (dict(critic=None), dict(state=None), dict(ld=J - 1), dict(B=-1), dict(mw=-1), dict(critic=_wrong(call.net, struct_size=short)),
               dict(critic=_wrong(call.net, w2=None)), dict(critic=_wrong(call.net, num_out=0)), dict(critic=_wrong(call.net, num_out=2)),
               dict(critic=_wrong(call.net, hidden1=-64)))
    unsupported = (dict(critic=_wrong(call.net, hidden1=257)), dict(critic=_wrong(call.net, hidden2=257)),
                   dict(critic=_wrong(call.net, num_state=4097, num_out=1), ld=4097), dict(critic=_wrong(call.net, num_state=65, num_out=65)))
    for ov in invalid + (dict(target=None), dict(ws=None), dict(grad=None), dict(loss=None), dict(ws=C.c_void_p(call.ws.data_ptr() + 4))):
        assert call.run_grad(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(OUTS), ov
    for ov in invalid + (dict(value=None),):
        assert call.run_value(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(("value_only",)), ov
    for ov in unsupported:
        assert call.run_grad(**ov) == nat.MDR_ERR_UNSUPPORTED and call.untouched(OUTS), ov
        assert call.run_value(**ov) == nat.MDR_ERR_UNSUPPORTED and call.untouched(("value_only",)), ov
    # the optional outputs may be missing
    assert call.run_grad(value=None, advantage=None) == nat.MDR_OK and call.untouched(("value", "advantage"))
    assert not bool(torch.isnan(call.out("grad")).any())
    torch.cuda.synchronize()


def _module(d):
    from mdr_amd.tarmac import TarMACCritic
    _, N, F = d["state"].shape
    critic = TarMACCritic(N, F, d["W1"].shape[0]).to(DEV)
    with torch.no_grad():
        for p, k in zip(critic.parameters(), R.PARAM_NAMES):
            p.copy_(_dev(d[k]))
    return critic


def test_python_calls_fill_grad_with_what_the_c_calls_wrote():
    from mdr_amd import tarmac_ppo
    M, B = 40, 33
    d = R.inputs(M, *R.NETS[5])
    idx = np.random.default_rng(2).integers(0, M, B).astype(np.int64)
    call = Call(d, index=_dev(idx))
    assert call.run_grad() == nat.MDR_OK
    want = call.results()
    critic = _module(d)
    params = list(critic.parameters())
    params[0].grad = torch.full_like(params[0], NAN)      # an existing gradient is overwritten, a missing one made
    assert params[2].grad is None
    state, target = _dev(d["state"]), _dev(d["target"])
    loss, adv, value = tarmac_ppo.critic_loss_backward(critic, state, target, index=_dev(idx), want_value=True)
    assert loss.dim() == 0 and loss.is_cuda and float(loss) == float(want["loss"])
    assert adv.shape == (B, 20) and np.array_equal(adv.cpu().numpy(), want["advantage"]) and np.array_equal(value.cpu().numpy(), want["value"])
    flat = torch.cat([p.grad.reshape(-1) for p in params]).cpu().numpy()
    assert np.array_equal(flat, want["grad"])
    assert params[2].grad.data_ptr() == critic._mdr_flat_grad.data_ptr() + 4 * (params[0].numel() + params[1].numel())      # views of one buffer
    loss2, adv2 = tarmac_ppo.critic_loss_backward(critic, state, target, index=_dev(idx))
    assert float(loss2) == float(loss) and torch.equal(adv2, adv)
    assert np.array_equal(tarmac_ppo.critic_value(critic, state, index=_dev(idx)).cpu().numpy(), want["value"])
    assert tarmac_ppo.critic_value(critic, state).shape == (M, 20)


def test_critic_supported_and_value_errors():
    from mdr_amd import tarmac_ppo
    from mdr_amd.tarmac import TarMACCritic
    critic = TarMACCritic(20, 51, 64).to(DEV)
    assert tarmac_ppo.critic_supported(critic) and tarmac_ppo.critic_supported(TarMACCritic(50, 51, 64).to(DEV))
    assert tarmac_ppo.critic_supported(TarMACCritic(5, 63, 97).to(DEV))
    wide, many, joint = TarMACCritic(20, 51, 300).to(DEV), TarMACCritic(65, 4, 64).to(DEV), TarMACCritic(64, 65, 64).to(DEV)
    assert not tarmac_ppo.critic_supported(wide) and not tarmac_ppo.critic_supported(many) and not tarmac_ppo.critic_supported(joint)
    assert not tarmac_ppo.critic_supported(TarMACCritic(20, 51, 64)) and not tarmac_ppo.critic_supported(torch.nn.Linear(4, 4).to(DEV))
    s, t = torch.zeros((4, 20, 51), device=DEV), torch.zeros((4, 20), device=DEV)
    with pytest.raises(ValueError, match="at most 256"):
        tarmac_ppo.critic_loss_backward(wide, s, t)
    with pytest.raises(ValueError, match="1 to 64"):
        tarmac_ppo.critic_value(many, s)
    with pytest.raises(ValueError, match="at most 4096"):
        tarmac_ppo.critic_value(joint, s)
    with pytest.raises(ValueError, match="state must"):
        tarmac_ppo.critic_loss_backward(critic, s[:, :, :50], t)
    with pytest.raises(ValueError, match="contiguous env-steps"):
        tarmac_ppo.critic_value(critic, torch.zeros((4, 20, 102), device=DEV)[:, :, ::2])
    with pytest.raises(ValueError, match="target must"):
        tarmac_ppo.critic_loss_backward(critic, s, t[:3])
    with pytest.raises(ValueError, match="index must"):
        tarmac_ppo.critic_loss_backward(critic, s, t, index=torch.zeros(3, dtype=torch.int32, device=DEV))
