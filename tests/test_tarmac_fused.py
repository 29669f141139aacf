"""The fragment order of mdr_tarmac_actor_t (include/mdr_policy.h) restated in numpy FROM THE HEADER, and the packer of
mdr_amd.tarmac held to it: unpack(pack(state_dict)) returns every weight and bias exactly.  No GPU."""
import numpy as np
import pytest
import torch

import mdr_amd
from mdr_amd import _native as nat
from mdr_amd.tarmac import FusedTarMACActor, TarMACActor, pack_tarmac_fragments

SHAPES = [(51, 64, 8, 16), (22, 8, 4, 4), (64, 48, 16, 32), (3, 64, 8, 16)]      # (F, H, K, V)


def nb(n):
    return -(-n // 16)


def rows(S, c0):
    """The input is read from memory: lane group g holds S consecutive floats of its agent's row."""
    return lambda s, g: c0 + g * S + s


def regs(s, g):
    """The input is the previous layer's accumulator."""
    return 16 * (s >> 2) + 4 * g + (s & 3)


def unpack_fragment(frag, S, nb_out, col, n_out, n_in, into=None):
    """frag[s][j][lane][i < w_j] = Wz[16 (4 j + i) + r][col(s, g)], 64 nbO floats per k-step, chunk j 256 j floats in.  -> (W [n_out,
    n_in] with the elements this fragment carries, the same-shaped count of how often each was seen); padding must be zero."""
    frag = np.asarray(frag).reshape(S, 64 * nb_out)
    W = np.zeros((n_out, n_in), dtype=np.float32) if into is None else into[0]
    seen = np.zeros((n_out, n_in), dtype=np.int64) if into is None else into[1]
    for s in range(S):
        for j in range(-(-nb_out // 4)):
            wj = min(4, nb_out - 4 * j)
            for lane in range(64):
                r, g = lane & 15, lane >> 4
                for i in range(wj):
                    val = frag[s, 256 * j + lane * wj + i]
                    row, c = 16 * (4 * j + i) + r, col(s, g)
                    if row < n_out and 0 <= c < n_in:
                        W[row, c] = val
                        seen[row, c] += 1
                    else:
                        assert val == 0.0, (s, j, lane, i)
    return W, seen


def unpack(p, F, H, K, V, hops, with_comm):
    """The five arrays -> a state_dict (the head's last layer as its difference)."""
    nbH, nbV, nbM = nb(H), nb(V), nb(H + V)
    sd = {}

    def take(arr, n):
        return arr[:n], arr[n:]

    def whole(name, frag, S, nbo, col, n_out, n_in):
        W, seen = unpack_fragment(frag, S, nbo, col, n_out, n_in)
        assert (seen == 1).all(), name
        sd[name] = W

    S1 = -(-F // 4)
    f, rest = take(p["frag_encode"], S1 * 64 * nbH)
    whole("obs2hidden.0.weight", f, S1, nbH, rows(S1, 0), H, F)      # columns past F: zeros
    whole("obs2hidden.2.weight", rest, 4 * nbH, nbH, regs, H, H)
    assert rest.size == 4 * nbH * 64 * nbH
    if with_comm:
        rest = p["frag_proj"]
        for n in ("query", "key", "value"):
            f, rest = take(rest, 4 * nbH * 64 * nbH)
            whole("comm.hidden2%s.0.weight" % n, f, 4 * nbH, nbH, regs, H, H)
        for n, dim, nbo in (("query", K, 1), ("key", K, 1), ("value", V, nbV)):
            f, rest = take(rest, 4 * nbH * 64 * nbo)
            whole("comm.hidden2%s.2.weight" % n, f, 4 * nbH, nbo, regs, dim, H)
        assert rest.size == 0
        if hops > 1:
            M = H + V
            f0, rest = take(p["frag_msg"], (V // 4) * 64 * nbM)
            f1, rest = take(rest, (H // 4) * 64 * nbM)
            acc = unpack_fragment(f0, V // 4, nbM, rows(V // 4, 0), M, M)      # the comm columns [0, V) of [comm, h]
            acc = unpack_fragment(f1, H // 4, nbM, rows(H // 4, V), M, M, into=acc)
            assert (acc[1] == 1).all()
            sd["comm.msg_state2state.0.weight"] = acc[0]
            whole("comm.msg_state2state.2.weight", rest, 4 * nbM, nbH, regs, H, M)
        else:
            assert p["frag_msg"] is None
        D = H + V
        whole("comm_hidden2action.0.weight", p["frag_head"], D // 4, nbH, rows(D // 4, 0), H, D)
    else:
        assert p["frag_proj"] is None and p["frag_msg"] is None
        whole("hidden2action.0.weight", p["frag_head"], H // 4, nbH, rows(H // 4, 0), H, H)
    c, head = ("comm.", "comm_hidden2action") if with_comm else (None, "hidden2action")
    rest = p["vec"]
    slots = [("obs2hidden.0.bias", 16 * nbH, H), ("obs2hidden.2.bias", 16 * nbH, H)]
    slots += [(c and c + "hidden2%s.0.bias" % n, 16 * nbH, H) for n in ("query", "key", "value")]
    slots += [(c and c + "hidden2query.2.bias", 16, K), (c and c + "hidden2key.2.bias", 16, K), (c and c + "hidden2value.2.bias", 16 * nbV, V)]
    slots += [(c and hops > 1 and c + "msg_state2state.0.bias", 16 * nbM, H + V), (c and hops > 1 and c + "msg_state2state.2.bias", 16 * nbH, H)]
    slots += [(head + ".0.bias", 16 * nbH, H), ("head.diff.weight", 16 * nbH, H), ("head.diff.bias", 4, 1)]
    for name, n, used in slots:
        f, rest = take(rest, n)
        if name:
            sd[name] = f[:used]
            assert not f[used:].any(), name
        else:
            assert not f.any()
    assert rest.size == 0
    return sd


def integer_actor(F, H, K, V, hops, with_comm):
    """Every element of every parameter a distinct small integer: a transposed or shifted element cannot hide."""
    actor = TarMACActor(F, num_key=K, num_value=V, hidden_state_size=H, num_hops=hops, with_comm=with_comm, attention="dense")
    base = 1
    with torch.no_grad():
        for p in actor.parameters():
            p.copy_(torch.arange(base, base + p.numel(), dtype=torch.float32).view_as(p))
            base += p.numel()
    assert base < 2 ** 24
    return actor


@pytest.mark.parametrize("hops,with_comm", [(1, True), (2, True), (1, False)])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_unpack_of_pack_returns_every_parameter(shape, hops, with_comm):
    F, H, K, V = shape
    actor = integer_actor(F, H, K, V, hops, with_comm)
    sd = {k: v.numpy() for k, v in actor.state_dict().items()}
    packed = pack_tarmac_fragments(sd, F, H, K, V, hops, with_comm)
    back = unpack(packed, F, H, K, V, hops, with_comm)
    head = "comm_hidden2action" if with_comm else "hidden2action"
    w3, b3 = sd.pop(head + ".2.weight"), sd.pop(head + ".2.bias")
    assert np.array_equal(back.pop("head.diff.weight"), w3[0] - w3[1]) and back.pop("head.diff.bias")[0] == b3[0] - b3[1]
    if hops == 1:      # a single hop never evaluates msg_state2state: not packed
        sd = {k: v for k, v in sd.items() if "msg_state2state" not in k}
    assert sorted(back) == sorted(sd)
    for name, w in sd.items():
        assert back[name].shape == w.shape and np.array_equal(back[name], w), name
    # the size helpers agree with the packed lengths
    mdr_amd.build_native()
    lib = nat.load()
    assert lib.mdr_tarmac_frag_encode_floats(F, H) == packed["frag_encode"].size
    assert lib.mdr_tarmac_frag_head_floats(H, V, int(with_comm)) == packed["frag_head"].size
    assert lib.mdr_tarmac_vec_floats(H, V) == packed["vec"].size
    if with_comm:
        assert lib.mdr_tarmac_frag_proj_floats(H, V) == packed["frag_proj"].size
        if hops > 1:
            assert lib.mdr_tarmac_frag_msg_floats(H, V) == packed["frag_msg"].size
    for arr in packed.values():
        assert arr is None or (arr.dtype == np.float32 and arr.size % 4 == 0)


def test_workspace_bytes_and_the_struct_mirror():
    import ctypes as C
    import os
    import re
    from mdr_amd.tarmac import MdrTarmacActor
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mdr_policy.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct mdr_tarmac_actor \{(.*?)\} mdr_tarmac_actor_t;", header, flags=re.S).group(1)
    fields = [re.sub(r"[\s\*]", "", d.strip().split()[-1]) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in MdrTarmacActor._fields_]
    mdr_amd.build_native()
    lib = nat.load()
    st = MdrTarmacActor()
    st.struct_size = C.sizeof(MdrTarmacActor)
    st.num_state, st.hidden, st.num_key, st.num_value, st.num_hops, st.with_comm = 51, 64, 8, 16, 1, 1
    assert lib.mdr_tarmac_actor_workspace_bytes(C.byref(st), 1000) == 1000 * 4 * (64 + 16 + 8 + 8 + 16)
    st.num_hops = 2
    assert lib.mdr_tarmac_actor_workspace_bytes(C.byref(st), 1000) == 1000 * 4 * (64 + 16 + 8 + 8 + 16 + 64)
    st.with_comm = 0
    assert lib.mdr_tarmac_actor_workspace_bytes(C.byref(st), 1000) == 1000 * 4 * 64
    st.struct_size -= 4
    assert lib.mdr_tarmac_actor_workspace_bytes(C.byref(st), 1000) == -1
    assert lib.mdr_tarmac_frag_encode_floats(65, 64) == -1 and lib.mdr_tarmac_frag_proj_floats(64, 64) == -1


@pytest.mark.parametrize("kw", [dict(num_key=32), dict(num_value=64), dict(num_obs=65), dict(num_action=3), dict(comm_mode="all")], ids=str)
def test_from_module_refuses_what_no_kernel_covers(kw):
    kw = dict(kw)
    F = kw.pop("num_obs", 51)
    mode = kw.pop("comm_mode", None)
    actor = TarMACActor(F, attention="dense", **kw)
    if mode is not None:
        actor.comm_mode = mode      # the constructor itself refuses the non-banded modes
    with pytest.raises(ValueError):
        FusedTarMACActor.from_module(actor)
    assert FusedTarMACActor.from_module(TarMACActor(51, attention="dense")) is not None
