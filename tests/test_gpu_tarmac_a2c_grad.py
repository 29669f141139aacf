"""mdr_tarmac_a2c_forward / _comm / _grad (include/mdr_policy.h) on the GPU, against the fp64 restatement and the derived rounding
bound of tests/tarmac_a2c_ref.py: every element of every output at worst |error| / bound <= 1."""
import ctypes as C

import numpy as np
import pytest
import torch

from mdr_amd import _native as nat
from tests import tarmac_a2c_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GRAD_OUTS = ("grad", "losses", "value", "advantage")
FWD_OUTS = ("logits", "value_only", "x")
COMM_OUTS = ("comm_out", "attn")
REF = R.SHAPES[4]      # the reference's sizes: N = 20, S = 128, C = 32
MID = R.SHAPES[2]      # N = 5: tiles straddle env-steps


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Call:
    """The three C calls on device copies of a case's inputs; every output and the workspace NaN-filled before each."""

    def __init__(self, d, max_workgroups=0, index=None, obs=None, ld_obs=None, comm=None, ld_comm=None, pad=0, ld_out=None):
        self.lib = nat.load()
        self.mw = max_workgroups
        M, N, F = d["obs"].shape
        Cc, S, K = d["comm"].shape[2], d["W2"].shape[0], d["Wq"].shape[0]
        self.N, self.F, self.C, self.S, self.K, self.M = N, F, Cc, S, K, M
        self.params = {k: _dev(d[k]) for k in R.PARAM_NAMES}
        self.net = nat.MdrTarmacA2CNet(C.sizeof(nat.MdrTarmacA2CNet), F, Cc, S, K, *[_ptr(self.params[k]) for k in R.PARAM_NAMES])
        self.obs = _dev(d["obs"]) if obs is None else obs
        self.comm = _dev(d["comm"]) if comm is None else comm
        self.ld_obs, self.ld_comm = F if ld_obs is None else ld_obs, Cc if ld_comm is None else ld_comm
        self.action, self.ret = _dev(d["action"]), _dev(d["ret"])
        self.index = index
        self.B = int(index.shape[0]) if index is not None else M
        self.vc, self.ec = float(R.VALUE_COEF), float(R.ENTROPY_COEF)
        self.G = int(self.lib.mdr_tarmac_a2c_grad_floats(C.byref(self.net)))
        nbytes = int(self.lib.mdr_tarmac_a2c_workspace_bytes(C.byref(self.net), self.B, N, max_workgroups))
        assert self.G == sum(d[k].size for k in R.REACHED) and nbytes > 0
        self.pad = pad      # canary elements on either side of every output
        self.ld_out = Cc if ld_out is None else ld_out
        self.ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
        R_ = self.B * N
        sizes = (("grad", self.G), ("losses", 3), ("value", self.B), ("advantage", R_), ("logits", 2 * R_), ("value_only", self.B),
                 ("x", R_ * S + 4), ("comm_out", R_ * self.ld_out), ("attn", R_ * N))
        self.bufs = {k: torch.empty(n + 2 * pad, dtype=torch.float32, device=DEV) for k, n in sizes}
        assert pad % 4 == 0      # x stays 16-byte aligned

    def out(self, k):
        b = self.bufs[k]
        return b[self.pad:b.numel() - self.pad]

    def _fill(self, keys):
        for k in keys:
            self.bufs[k].fill_(NAN)

    def run_grad(self, **ov):
        self.ws.fill_(NAN)
        self._fill(GRAD_OUTS)
        a = dict(net=C.byref(self.net), obs=_ptr(self.obs), ld_obs=self.ld_obs, comm=_ptr(self.comm), ld_comm=self.ld_comm,
                 action=_ptr(self.action), ret=_ptr(self.ret), index=_ptr(self.index), B=self.B, N=self.N, vc=self.vc, ec=self.ec, mw=self.mw,
                 ws=_ptr(self.ws), grad=_ptr(self.out("grad")), losses=_ptr(self.out("losses")), value=_ptr(self.out("value")),
                 advantage=_ptr(self.out("advantage")))
        a.update(ov)
        return self.lib.mdr_tarmac_a2c_grad(a["net"], a["obs"], a["ld_obs"], a["comm"], a["ld_comm"], a["action"], a["ret"], a["index"], a["B"],
                                            a["N"], C.c_float(a["vc"]), C.c_float(a["ec"]), a["mw"], a["ws"], a["grad"], a["losses"], a["value"],
                                            a["advantage"], _stream())

    def run_forward(self, **ov):
        self._fill(FWD_OUTS)
        a = dict(net=C.byref(self.net), obs=_ptr(self.obs), ld_obs=self.ld_obs, comm=_ptr(self.comm), ld_comm=self.ld_comm,
                 index=_ptr(self.index), B=self.B, N=self.N, mw=self.mw, ws=None, logits=_ptr(self.out("logits")),
                 value=_ptr(self.out("value_only")), x=_ptr(self.out("x")))
        a.update(ov)
        return self.lib.mdr_tarmac_a2c_forward(a["net"], a["obs"], a["ld_obs"], a["comm"], a["ld_comm"], a["index"], a["B"], a["N"], a["mw"],
                                               a["ws"], a["logits"], a["value"], a["x"], _stream())

    def run_comm(self, **ov):
        """The attention of the B env-steps on the x run_forward left."""
        self._fill(COMM_OUTS)
        a = dict(net=C.byref(self.net), x=_ptr(self.out("x")), E=self.B, N=self.N, mw=self.mw, out=_ptr(self.out("comm_out")), ld=self.ld_out,
                 attn=_ptr(self.out("attn")))
        a.update(ov)
        return self.lib.mdr_tarmac_a2c_comm(a["net"], a["x"], a["E"], a["N"], a["mw"], a["out"], a["ld"], a["attn"], _stream())

    def run_all(self):
        assert self.run_grad() == nat.MDR_OK and self.run_forward() == nat.MDR_OK and self.run_comm() == nat.MDR_OK
        return self.results()

    def results(self):
        B, N, S, Cc = self.B, self.N, self.S, self.C
        R_ = B * N
        r = {k: self.out(k).cpu().numpy() for k in ("grad", "losses", "value", "value_only")}
        r["advantage"] = self.out("advantage").cpu().numpy().reshape(B, N)
        r["logits"] = self.out("logits").cpu().numpy().reshape(R_, 2)
        r["x"] = self.out("x").cpu().numpy()[:R_ * S].reshape(R_, S)
        r["x_tail"] = self.out("x").cpu().numpy()[R_ * S:]
        co = self.out("comm_out").cpu().numpy().reshape(R_, self.ld_out)
        r["comm_out"], r["comm_gap"] = co[:, :Cc].reshape(B, N, Cc), co[:, Cc:]
        r["attn"] = self.out("attn").cpu().numpy().reshape(B, N, N)
        # the workspace: h1 | x | dx | dz1 [Rp][Sp], logits | dl [Rp][2], xbar | a | da | dxbar / N [Bp][Sp], dV [Bp], terms [Bp][4]
        Rp, Bp, Sp = (R_ + 15) // 16 * 16, (B + 15) // 16 * 16, (S + 15) // 16 * 16
        ws = self.ws.cpu().numpy()
        off = 0
        for name, rows, width in (("h1", Rp, Sp), ("ws_x", Rp, Sp), ("dx", Rp, Sp), ("dz1", Rp, Sp), ("ws_logits", Rp, 2), ("dl", Rp, 2),
                                  ("xbar", Bp, Sp), ("a", Bp, Sp), ("da", Bp, Sp), ("dxm", Bp, Sp), ("dV", Bp, 1), ("terms", Bp, 4)):
            r["ws/" + name] = ws[off:off + rows * width].reshape(rows, width)
            off += rows * width
        r["ws_floats"] = off
        return r

    def untouched(self, keys):
        return all(bool(torch.isnan(self.bufs[k]).all()) for k in keys)

    def canaries_intact(self):
        p = self.pad
        return all(bool(torch.isnan(torch.cat([b[:p], b[b.numel() - p:]])).all()) for b in self.bufs.values())


WORST = {}
BITS = ("grad", "losses", "value", "advantage", "logits", "x", "comm_out", "attn", "value_only")


def _check(got, r, label, keys=R.FLOAT_KEYS):
    for k in keys:
        w = R.worst(got[k], r["ref"][k], r["bound"][k])
        WORST[k] = max(WORST.get(k, 0.0), w)
        print("%s %-9s worst |error| / bound = %.3f" % (label, k, w))
        assert np.isfinite(np.asarray(got[k])).all(), (label, k)
        assert w <= 1.0, (label, k, w)


def _bits_equal(ra, rb, keys=BITS):
    for k in keys:
        assert np.array_equal(np.asarray(ra[k]).view(np.uint32), np.asarray(rb[k]).view(np.uint32)), k


def _zeros_past_the_batch(got, B, N, S):
    R_ = B * N
    for k in ("h1", "ws_x", "dx", "dz1", "ws_logits", "dl"):
        assert not got["ws/" + k][R_:].any(), k
    for k in ("xbar", "a", "da", "dxm", "dV", "terms"):
        assert not got["ws/" + k][B:].any(), k
    for k in ("h1", "ws_x", "dx", "dz1", "xbar", "a", "da", "dxm"):
        assert not got["ws/" + k][:, S:].any(), k
    assert np.isfinite(got["ws/dz1"]).all() and np.isfinite(got["ws/terms"]).all()


SWEEP = [(B,) + s for s in R.SHAPES for B in R.STEPS]


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "B%d-N%d-F%d-C%d-S%d-K%d" % c)
def test_sweep_matches_fp64_within_the_bound(case, record_property):
    r = R.reference(*case)
    call = Call(r["inputs"])
    got = call.run_all()
    _check(got, r, "B%d N%d F%d C%d S%d K%d" % case)
    # the forward alone: the same bits as the update's
    assert np.array_equal(got["value_only"].view(np.uint32), got["value"].view(np.uint32))
    assert np.array_equal(got["logits"].view(np.uint32), got["ws/ws_logits"][:case[0] * case[1]].view(np.uint32))
    assert np.array_equal(got["x"].view(np.uint32), got["ws/ws_x"][:case[0] * case[1], :case[4]].view(np.uint32))
    assert np.isnan(got["x_tail"]).all()
    _zeros_past_the_batch(got, case[0], case[1], case[4])
    record_property("worst_ratio", max(WORST.values()))
    print("worst |error| / bound so far: " + ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def _case(d, index=None):
    return dict(inputs=d, ref=R.evaluate(d, index=index), bound=R.bound(d, index=index))


@pytest.mark.parametrize("shape,B,mw", [(MID, 33, 2), (MID, 33, 1), (REF, 17, 2), (R.SHAPES[3], 33, 2), (R.SHAPES[0], 33, 1), (R.SHAPES[6], 5, 2)],
                         ids=str)
def test_few_workgroups_give_the_bits_of_the_default_grid(shape, B, mw):
    """max_workgroups = 2 (or 1): every pass loops over its tiles, env-steps, envs and weight blocks."""
    r = _case(R.inputs(B, *shape))
    ra, rb = Call(r["inputs"], max_workgroups=mw).run_all(), Call(r["inputs"]).run_all()
    _bits_equal(ra, rb)
    _check(ra, r, "%s B%d max_workgroups=%d" % (shape, B, mw))


def test_one_tile_beyond_a_full_pass_of_the_library_grid():
    """The library's own grid loops: as many tiles of 16 rows as its cap and one more (one row of it); the bits of a grid of two."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    N = MID[0]
    B = -(-(16 * min(cus, 512) + 1) // N)
    assert 16 * min(cus, 512) < B * N <= 16 * (min(cus, 512) + 1) and B < 10 ** 4
    d = R.inputs(B, *MID)
    ra, rb = Call(d).run_all(), Call(d, max_workgroups=2).run_all()
    _bits_equal(ra, rb)
    _check(ra, _case(d), "B%d own grid" % B)


def test_index_equals_the_gathered_copy_bit_for_bit():
    M, B = 33, 21
    d = R.inputs(M, *REF)
    idx = np.random.default_rng(5).integers(0, M, B)
    idx[:4] = [30, 3, 30, 3]      # repeats, out of order
    gathered = dict(d, obs=d["obs"][idx], comm=d["comm"][idx], ret=d["ret"][idx], action=d["action"][idx])
    ra, rb = Call(d, index=_dev(idx.astype(np.int64))).run_all(), Call(gathered).run_all()
    _bits_equal(ra, rb)
    _check(ra, _case(d, index=idx), "index")


def test_strided_rows_and_canaries():
    B, shape = 17, R.SHAPES[2]
    N, F, Cc, S, K = shape
    r = R.reference(B, *shape)
    wide_o = torch.full((B * N, F + 13), NAN, dtype=torch.float32, device=DEV)
    wide_o[:, 5:5 + F] = _dev(r["inputs"]["obs"]).reshape(B * N, F)
    wide_c = torch.full((B * N, Cc + 7), NAN, dtype=torch.float32, device=DEV)
    wide_c[:, 3:3 + Cc] = _dev(r["inputs"]["comm"]).reshape(B * N, Cc)
    call = Call(r["inputs"], obs=wide_o[:, 5:5 + F], ld_obs=F + 13, comm=wide_c[:, 3:3 + Cc], ld_comm=Cc + 7, pad=64, ld_out=Cc + 9)
    got = call.run_all()
    assert call.canaries_intact()
    assert np.isnan(got["comm_gap"]).all()      # the slab between the rows of comm_out is not written
    _check(got, r, "strided")
    assert np.array_equal(got["value_only"].view(np.uint32), got["value"].view(np.uint32))


def test_two_calls_give_equal_bits():
    r = R.reference(17, *REF)
    call = Call(r["inputs"], max_workgroups=3)
    first = call.run_all()
    _bits_equal(first, call.run_all())


def test_nan_in_ret_reaches_losses_and_advantage_and_stays_out_of_value():
    d = R.inputs(17, *MID)
    call = Call(d)
    call.ret[11, 1] = NAN
    assert call.run_grad() == nat.MDR_OK
    got = call.results()
    assert np.isnan(got["losses"][:2]).all() and not np.isnan(got["losses"][2])
    assert np.isnan(got["advantage"]).sum() == 1 and np.isnan(got["advantage"][11, 1])
    assert np.isnan(got["value"]).sum() == 0
    s = R.param_slices(MID[1], MID[2], MID[3])
    assert np.isnan(got["grad"][s["bc2"]]).all() and np.isnan(got["grad"][s["Wd"]]).all()


def test_zero_steps_write_zeros():
    call = Call(R.inputs(16, *MID))
    assert call.run_forward(B=0) == nat.MDR_OK and call.untouched(FWD_OUTS)
    assert call.run_comm(E=0) == nat.MDR_OK and call.untouched(COMM_OUTS)
    assert call.run_grad(B=0) == nat.MDR_OK
    assert bool((call.out("grad") == 0).all()) and bool((call.out("losses") == 0).all()) and call.untouched(("value", "advantage"))


def _wrong(net, **fields):
    twin = nat.MdrTarmacA2CNet.from_buffer_copy(net)
    for k, v in fields.items():
        setattr(twin, k, v)
    return C.byref(twin)


def test_refusals_leave_every_output_untouched():
    call = Call(R.inputs(17, *MID))
    assert call.run_forward() == nat.MDR_OK      # an x for the attention's refusals
    net = call.net
    short = net.struct_size - 8
    bad_net = (dict(net=None), dict(net=_wrong(net, struct_size=short)), dict(net=_wrong(net, state_size=0)), dict(net=_wrong(net, num_obs=-3)),
               dict(net=_wrong(net, num_key=0)))
    rows_invalid = bad_net + (dict(obs=None), dict(comm=None), dict(ld_obs=call.F - 1), dict(ld_comm=call.C - 1), dict(B=-1), dict(N=0),
                              dict(mw=-1), dict(net=_wrong(net, common_w2=None)), dict(net=_wrong(net, dist_w=None)))
    unsupported = (dict(N=65), dict(net=_wrong(net, state_size=132)), dict(net=_wrong(net, num_comm=36), ld_comm=36),
                   dict(net=_wrong(net, num_key=20)), dict(net=_wrong(net, num_obs=129), ld_obs=129), dict(net=_wrong(net, state_size=34)),
                   dict(net=_wrong(net, num_comm=6)), dict(net=_wrong(net, num_key=6)))
    for ov in rows_invalid + (dict(action=None), dict(ret=None), dict(ws=None), dict(grad=None), dict(losses=None),
                              dict(ws=C.c_void_p(call.ws.data_ptr() + 4))):
        assert call.run_grad(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(GRAD_OUTS), ov
    for ov in rows_invalid + (dict(logits=None), dict(value=None), dict(x=None), dict(x=C.c_void_p(call.out("x").data_ptr() + 4))):
        assert call.run_forward(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(FWD_OUTS), ov
    for ov in bad_net + (dict(x=None), dict(out=None), dict(ld=call.C - 1), dict(E=-1), dict(N=0), dict(mw=-1), dict(net=_wrong(net, key_w=None))):
        assert call.run_comm(**ov) == nat.MDR_ERR_INVALID, ov
        assert call.untouched(COMM_OUTS), ov
    for ov in unsupported:
        assert call.run_grad(**ov) == nat.MDR_ERR_UNSUPPORTED and call.untouched(GRAD_OUTS), ov
        assert call.run_forward(**ov) == nat.MDR_ERR_UNSUPPORTED and call.untouched(FWD_OUTS), ov
        ovc = dict({k: v for k, v in ov.items() if k in ("net", "N")}, ld=64)      # a row stride every num_comm here fits
        assert call.run_comm(**ovc) == nat.MDR_ERR_UNSUPPORTED and call.untouched(COMM_OUTS), ov
    assert call.lib.mdr_tarmac_a2c_grad_floats(_wrong(net, state_size=132)) == -1
    assert call.lib.mdr_tarmac_a2c_workspace_bytes(C.byref(net), 4, 65, 0) == -1
    # the optional outputs may be missing; the forward takes the workspace where no x is asked for
    assert call.run_grad(value=None, advantage=None) == nat.MDR_OK and call.untouched(("value", "advantage"))
    assert not bool(torch.isnan(call.out("grad")).any())
    want = call.out("value").clone()
    assert call.run_grad() == nat.MDR_OK
    assert call.run_forward(x=None, ws=_ptr(call.ws)) == nat.MDR_OK and call.untouched(("x",))
    assert torch.equal(call.out("value_only"), call.out("value"))
    torch.cuda.synchronize()


def test_attention_rows_sum_to_one_and_a_single_agent_hears_itself():
    r = R.reference(17, *REF)
    got = Call(r["inputs"]).run_all()
    err = np.abs(got["attn"].astype(np.float64).sum(axis=2) - 1.0)
    assert (err <= r["bound"]["attn"].sum(axis=2) + R.U).all()
    one = R.reference(3, *R.SHAPES[0])      # N = 1
    call = Call(one["inputs"])
    g1 = call.run_all()
    assert (g1["attn"] == 1.0).all()
    d = one["inputs"]
    v = R.evaluate(d, np.float64)
    assert R.worst(g1["comm_out"], v["comm_out"], one["bound"]["comm_out"]) <= 1.0
    # comm_out = v exactly: attn = 1, one product and one sum with zero
    vv = (torch.from_numpy(g1["x"]).double() @ torch.from_numpy(d["Wv"]).double().T + torch.from_numpy(d["bv"]).double()).numpy()
    assert np.abs(g1["comm_out"].reshape(3, -1) - vv).max() <= (one["bound"]["comm_out"]).max()
    assert call.run_comm(attn=None) == nat.MDR_OK and call.untouched(("attn",))
