"""MDR_TARMAC_BF16X3 without a GPU: the bf16 split, the packer of mdr_amd.tarmac held to the fragment order of include/mdr_policy.h
(restated in tests/tarmac_bf16_ref.py), the header and its ctypes mirror, and the proof that the bf16x3 probability contract tells
the right arithmetic from the three forms that drop a cross term - on every recorded reference case and on every synthetic input of
tests/test_gpu_tarmac_bf16.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mdr_amd
from mdr_amd import _native as nat
from mdr_amd.tarmac import FusedTarMACActor, MdrTarmacActor, TarMACActor, pack_tarmac_fragments
from tests import actor_ref as ar
from tests import tarmac_bf16_ref as br
from tests import tarmac_ref as tr

CASES = tr.load_cases()
SYNTHETIC = br.synthetic_inputs()


# ---------------------------------------------------------------------------------------------------------------- 1. the split
def test_split_reproduces_x_to_two_to_the_minus_16_and_rounds_ties_to_even():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.standard_normal(20000) * 10.0 ** rng.integers(-6, 6, 20000), [0.0, 1.0, -1.0, 3.0e38, 1e-30]]).astype(np.float32)
    head, tail = br.split(x)
    err = np.abs(head.astype(np.float64) + tail.astype(np.float64) - x.astype(np.float64))
    assert (err <= 2.0 ** -16 * np.abs(x.astype(np.float64))).all()
    # ties: 1 + 2^-8 lies halfway between the bf16 neighbours 1 (even) and 1 + 2^-7 (odd); 1 + 3 * 2^-8 halfway between 1 + 2^-7 and
    # 1 + 2^-6 (even); one float32 ulp either side of a tie goes to the nearer neighbour
    bits = lambda v: int(br.bf16_bits(np.array([v], dtype=np.float32))[0])
    assert bits(1.0 + 2.0 ** -8) == 0x3F80 and bits(1.0 + 3 * 2.0 ** -8) == 0x3F82
    assert bits(-(1.0 + 2.0 ** -8)) == 0xBF80 and bits(-(1.0 + 3 * 2.0 ** -8)) == 0xBF82
    assert bits(np.nextafter(np.float32(1.0 + 2.0 ** -8), np.float32(2))) == 0x3F81
    assert bits(np.nextafter(np.float32(1.0 + 3 * 2.0 ** -8), np.float32(0))) == 0x3F81
    assert bits(0.0) == 0 and bits(1.0) == 0x3F80


def test_split_bits_are_those_of_the_plain_actors_bf16x3_packer():
    """policy.py's packer: head = w.to(bfloat16), tail = (w - head.float()).to(bfloat16)."""
    from mdr_amd.tarmac import bf16_split
    rng = np.random.default_rng(6)
    x = (rng.standard_normal(50000) * 10.0 ** rng.integers(-4, 4, 50000)).astype(np.float32)
    x[:4] = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 0.0]
    t = torch.from_numpy(x)
    head = t.to(torch.bfloat16)
    tail = (t - head.float()).to(torch.bfloat16)
    want = (head.view(torch.int16).numpy().view(np.uint16), tail.view(torch.int16).numpy().view(np.uint16))
    h, l = br.split(x)
    for got in ((br.bf16_bits(x), br.bf16_bits(x - h)), bf16_split(x)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(h, head.float().numpy()) and np.array_equal(l, tail.float().numpy())


# -------------------------------------------------------------------------------------------------- 2. the packer, round trip
ROUND_TRIP = [(51, 64, 8, 16, 2, True), (64, 48, 16, 32, 2, True), (3, 64, 4, 4, 1, True), (22, 64, 8, 16, 1, False)]


def _random_actor(F, H, K, V, hops, with_comm):
    torch.manual_seed(F + H + K + V)
    actor = TarMACActor(F, num_key=K, num_value=V, hidden_state_size=H, num_hops=hops, with_comm=with_comm, attention="dense")
    with torch.no_grad():
        for p in actor.parameters():      # no zeros: a weight that went missing cannot pass as padding
            p.copy_(torch.where(p == 0, torch.ones_like(p), p))
    return actor


def _struct(F, H, K, V, hops, with_comm, precision):
    st = MdrTarmacActor()
    st.struct_size = C.sizeof(MdrTarmacActor)
    st.num_state, st.hidden, st.num_key, st.num_value, st.num_hops, st.with_comm, st.precision = F, H, K, V, hops, int(with_comm), precision
    return st


@pytest.mark.parametrize("shape", ROUND_TRIP, ids=str)
def test_bf16_packer_round_trip_and_sizes(shape):
    F, H, K, V, hops, with_comm = shape
    actor = _random_actor(*shape)
    sd = {k: v.numpy() for k, v in actor.state_dict().items()}
    packed = pack_tarmac_fragments(sd, F, H, K, V, hops, with_comm, precision="bf16x3")
    back = br.unpack(packed, F, H, K, V, hops, with_comm)      # asserts: every weight once, all padding zero, exact lengths
    head = "comm_hidden2action" if with_comm else "hidden2action"
    layers = ["obs2hidden.0", "obs2hidden.2", head + ".0"]
    if with_comm:
        layers += ["comm.hidden2%s.%d" % (n, i) for n in ("query", "key", "value") for i in (0, 2)]
        if hops > 1:
            layers += ["comm.msg_state2state.0", "comm.msg_state2state.2"]
    assert sorted(back) == sorted(n + ".weight" for n in layers)
    for name, (h, l) in back.items():
        w = sd[name]
        wh, wl = br.split(w)
        assert h.shape == w.shape and np.array_equal(br.bf16_value(h), wh) and np.array_equal(br.bf16_value(l), wl), name
        assert h.any() and l.any()
    # the fp32 parts are untouched by the precision, and the default is the fp32 packing
    plain = pack_tarmac_fragments(sd, F, H, K, V, hops, with_comm)
    fp32 = pack_tarmac_fragments(sd, F, H, K, V, hops, with_comm, precision="fp32")
    assert np.array_equal(packed["vec"], plain["vec"]) and packed["vec"].dtype == np.float32
    assert sorted(plain) == sorted(fp32) == sorted(packed)
    for n in plain:
        assert (plain[n] is None and fp32[n] is None) or (plain[n].dtype == fp32[n].dtype == np.float32 and np.array_equal(plain[n], fp32[n])), n
    # the size helper: host only
    mdr_amd.build_native()
    lib = nat.load()
    st = _struct(F, H, K, V, hops, with_comm, 1)
    parts = ("frag_encode", "frag_proj", "frag_msg", "frag_head")
    for part, n in enumerate(parts):
        if packed[n] is not None:
            assert lib.mdr_tarmac_frag_words(C.byref(st), part) == packed[n].size, n
            assert packed[n].size % 512 == 0
    st.precision = 0
    assert lib.mdr_tarmac_frag_words(C.byref(st), 0) == lib.mdr_tarmac_frag_encode_floats(F, H)
    assert lib.mdr_tarmac_frag_words(C.byref(st), 1) == lib.mdr_tarmac_frag_proj_floats(H, V)
    assert lib.mdr_tarmac_frag_words(C.byref(st), 2) == lib.mdr_tarmac_frag_msg_floats(H, V)
    assert lib.mdr_tarmac_frag_words(C.byref(st), 3) == lib.mdr_tarmac_frag_head_floats(H, V, int(with_comm))
    for part, n in enumerate(parts):
        if plain[n] is not None:
            assert lib.mdr_tarmac_frag_words(C.byref(st), part) == plain[n].size, n


def test_frag_words_refusals_and_the_lds_table():
    mdr_amd.build_native()
    lib = nat.load()
    st = _struct(51, 64, 8, 16, 2, True, 1)
    # the reference's sizes: 46 pairs (encode + proj) and 57 (msg + proj) of 2 KiB; the largest covered shape: 48 and 62
    words = [lib.mdr_tarmac_frag_words(C.byref(st), p) for p in range(4)]
    assert (words[0] + words[1]) * 4 == 46 * 2048 and (words[2] + words[1]) * 4 == 57 * 2048 and words[3] * 4 == 12 * 2048
    big = _struct(64, 64, 16, 32, 2, True, 1)
    words = [lib.mdr_tarmac_frag_words(C.byref(big), p) for p in range(4)]
    assert (words[0] + words[1]) * 4 == 48 * 2048 and (words[2] + words[1]) * 4 == 62 * 2048
    assert lib.mdr_tarmac_frag_words(C.byref(st), 4) == -1 and lib.mdr_tarmac_frag_words(C.byref(st), -1) == -1
    assert lib.mdr_tarmac_frag_words(None, 0) == -1
    for field, value in (("precision", 2), ("precision", -1), ("num_state", 65), ("hidden", 62), ("num_key", 32), ("num_value", 64),
                         ("struct_size", C.sizeof(MdrTarmacActor) - 4)):
        bad = MdrTarmacActor.from_buffer_copy(st)
        setattr(bad, field, value)
        assert lib.mdr_tarmac_frag_words(C.byref(bad), 0) == -1, field
    # mdr_tarmac_actor_workspace_bytes does not depend on the precision
    st0 = _struct(51, 64, 8, 16, 2, True, 0)
    assert lib.mdr_tarmac_actor_workspace_bytes(C.byref(st), 1000) == lib.mdr_tarmac_actor_workspace_bytes(C.byref(st0), 1000) == 1000 * 4 * 176


# ------------------------------------------------------------------------------------------------------ 3. header and mirror
def test_header_has_precision_where_reserved0_was_and_the_mirror_agrees():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdr_policy.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct mdr_tarmac_actor \{(.*?)\} mdr_tarmac_actor_t;", header, flags=re.S).group(1)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    fields = [re.sub(r"[\s\*]", "", d.split()[-1]) for d in decls]
    assert fields == ["struct_size", "num_state", "hidden", "num_key", "num_value", "nb_comm", "mode", "num_hops", "with_comm", "defect_prob",
                      "greedy", "precision", "frag_encode", "frag_proj", "frag_msg", "frag_head", "vec"]
    assert decls[11] == "int32_t precision" and "reserved0" not in body
    assert fields == [f[0] for f in MdrTarmacActor._fields_]
    assert dict(MdrTarmacActor._fields_)["precision"] is C.c_int32
    assert MdrTarmacActor.precision.offset == 44 and C.sizeof(MdrTarmacActor) == 88      # the layout did not move
    assert re.search(r"MDR_TARMAC_FP32\s*=\s*0", header) and re.search(r"MDR_TARMAC_BF16X3\s*=\s*1", header)
    assert re.search(r"#define MDR_ABI_VERSION 5\b", open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdr.h")).read())


def test_precision_option():
    actor = TarMACActor(51, attention="dense")
    assert FusedTarMACActor.from_module(actor).precision == "fp32" and FusedTarMACActor(actor).precision == "fp32"
    assert FusedTarMACActor.from_module(actor, precision="bf16x3").precision == "bf16x3"
    assert FusedTarMACActor(actor, precision="bf16x3").precision == "bf16x3"
    for bad in ("fp16", "bf16", None, 1):
        with pytest.raises(ValueError):
            FusedTarMACActor.from_module(actor, precision=bad)
    with pytest.raises(ValueError):
        pack_tarmac_fragments(actor.state_dict(), 51, 64, 8, 16, precision="fp16")
    with pytest.raises(ValueError):      # the shape refusals are those of the fp32 form
        FusedTarMACActor.from_module(TarMACActor(51, num_key=32, attention="dense"), precision="bf16x3")


# ------------------------------------------------------------------------------------------- 4. the contract discriminates
def _judge(what, sd, obs, ref64, nb_comm, hops, **kw):
    p = br.actor_forward_bf16x3(sd, obs, nb_comm, hops, **kw)
    good = ar.contract_ratio(p, ref64, True).max()
    worst = {name: ar.contract_ratio(br.actor_forward_bf16x3(sd, obs, nb_comm, hops, **kw, **v), ref64, True).max() for name, v in br.VARIANTS.items()}
    print("%s: bf16x3 %.4f of the contract; %s" % (what, good, ", ".join("%s %.2f" % kv for kv in worst.items())))
    assert good <= 1.0
    for name, ratio in worst.items():
        assert ratio > 1.0, name


@pytest.mark.parametrize("name", sorted(CASES))
def test_contract_discriminates_on_the_recorded_cases(name):
    case = CASES[name]
    _judge(name, case["sd"], case["obs"], case["probs"], case["c"], case["hops"], mode=case["mode"], with_comm=case["with_comm"])


@pytest.mark.parametrize("name", sorted(SYNTHETIC))
def test_contract_discriminates_on_the_synthetic_inputs_of_the_gpu_tests(name):
    actor, obs, ref64, ref_kw = br.build_input(SYNTHETIC[name])
    _judge(name, br.state_dict(actor), obs.numpy(), ref64, 10, actor.num_hops, **ref_kw)


def test_contract_discriminates_on_the_grid_stride_input():
    """At the 256 CUs of an MI355X: the envs the GPU test holds to the fp64 reference."""
    E, _, envs = br.grid_stride_input(256)
    actor = br.make_actor(51, hops=br.GRID_HOPS)
    obs = br.grid_stride_obs(E)[envs].numpy()
    sd = br.state_dict(actor)
    _judge("grid stride", sd, obs, tr.actor_forward(sd, obs, 10, br.GRID_HOPS), 10, br.GRID_HOPS)
