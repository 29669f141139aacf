"""What MDR_TARMAC_BF16X3 computes (include/mdr_policy.h, csrc/mdr_tarmac_mlp_bf16.hip), restated in numpy on the CPU: the bf16 head /
tail split, an emulation of the whole actor forward in exactly that arithmetic - with switches for the three wrong variants that drop
a cross term - the unpacker of the bf16 fragments written FROM THE HEADER, and the synthetic inputs of tests/test_gpu_tarmac_bf16.py,
built here so that tests/test_tarmac_bf16.py can judge them without a kernel.

The tolerance is the project's bf16x3 probability contract, actor_ref.contract_ratio(p, ref64, True) <= 1, against the fp64 forward of
tests/tarmac_ref.py.  Nothing here is fitted to what a kernel returns."""
import numpy as np

from tests import tarmac_ref as tr


# ---- the split
def bf16_bits(x):
    """float32 -> the 16 bits of bf16(x), round to nearest even (finite x)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def split(x):
    """float32 x -> (head, tail) as float32 values: head = bf16(x), tail = bf16(x - head)."""
    x = np.asarray(x, dtype=np.float32)
    head = bf16_value(bf16_bits(x))
    return head, bf16_value(bf16_bits(x - head))


# ---- the emulated forward
def _linear(sd, name, x, wl_xh=True, wh_xl=True):
    """b + Wh xh [+ Wl xh] [+ Wh xl] with every product and sum in float32."""
    wh, wl = split(sd[name + ".weight"])
    xh, xl = split(x)
    y = xh @ wh.T
    if wl_xh:
        y = y + xh @ wl.T
    if wh_xl:
        y = y + xl @ wh.T
    return (y + sd[name + ".bias"].astype(np.float32)).astype(np.float32)


def _mlp(sd, prefix, x, act, **variant):
    h = _linear(sd, prefix + ".0", x, **variant)
    h = np.maximum(h, np.float32(0)) if act == "relu" else np.tanh(h)
    return _linear(sd, prefix + ".2", h.astype(np.float32), **variant)


def actor_forward_bf16x3(sd, obs, nb_comm, num_hops=1, mode=tr.NEIGHBOURS, with_comm=True, dead=None, wl_xh=True, wh_xl=True):
    """tarmac_ref.actor_forward in the arithmetic of MDR_TARMAC_BF16X3: every weight and every input of a matrix layer rounded to a
    bf16 head and tail, the three products summed, everything else - biases, activations, the attention, the head's last layer as
    the dot with W3[0] - W3[1], the two-logit softmax - in float32.  obs [E, N, F] -> float32 probabilities [E, N, 2].
    ``wl_xh=False`` / ``wh_xl=False``: the wrong variants without that cross term; both False: heads only."""
    sd = {n: np.asarray(w, dtype=np.float32) for n, w in sd.items()}
    v = dict(wl_xh=wl_xh, wh_xl=wh_xl)
    x = _mlp(sd, "obs2hidden", np.asarray(obs, dtype=np.float32), "relu", **v)
    if not with_comm:
        head, row = "hidden2action", x
    else:
        h, comm = x, None
        for hop in range(num_hops):
            if hop > 0:
                h = _mlp(sd, "comm.msg_state2state", np.concatenate([comm, h], axis=2), "tanh", **v)
            key, value, query = (_mlp(sd, "comm.hidden2" + n, h, "tanh", **v) for n in ("key", "value", "query"))
            d = dead[hop] if dead is not None else None
            comm = tr.band_attention(query, key, value, nb_comm, mode, d, dtype=np.float32)[0].astype(np.float32)
        head, row = "comm_hidden2action", np.concatenate([x, comm], axis=2)
    t = np.maximum(_linear(sd, head + ".0", row, **v), np.float32(0))
    w3, b3 = sd[head + ".2.weight"], sd[head + ".2.bias"]
    d = (t @ (w3[0] - w3[1]) + (b3[0] - b3[1])).astype(np.float32)
    one = np.float32(1)
    with np.errstate(over="ignore"):
        return np.stack([one / (one + np.exp(-d)), one / (one + np.exp(d))], axis=-1).astype(np.float32)


VARIANTS = {"no Wl.xh": dict(wl_xh=False), "no Wh.xl": dict(wh_xl=False), "heads only": dict(wl_xh=False, wh_xl=False)}


# ---- the fragments, from the header:
#   frag[s][mb < nbO][t][lane][j < 8] = split_t(Wz[16 mb + r][col(s, g, j)]),  t = 0 head / 1 tail, 512 words per (s, mb) pair,
#   bf16 j of a lane in the low (even j) / high (odd j) half of word j / 2
#   rows(n, c0): c0 + 32 s + 8 g + j, S = ceil(n / 32), zero where 32 s + 8 g + j >= n
#   regs(nbI):   16 (2 s + (j >> 2)) + 4 g + (j & 3), S = ceil(nbI / 2), zero where 2 s + (j >> 2) >= nbI and past the layer's inputs
def nb(n):
    return -(-n // 16)


def rows(n, c0):
    return -(-n // 32), lambda s, g, j: c0 + 32 * s + 8 * g + j if 32 * s + 8 * g + j < n else None


def regs(nb_in):
    return -(-nb_in // 2), lambda s, g, j: 16 * (2 * s + (j >> 2)) + 4 * g + (j & 3) if 2 * s + (j >> 2) < nb_in else None


def unpack_fragment(words, nb_out, source, n_out, n_in, into=None):
    """The words of one layer -> (head bits, tail bits, seen) as [n_out, n_in] arrays; every element that is no weight must be an exact
    zero in both halves.  -> the number of words the layer took."""
    S, col = source
    halves = np.ascontiguousarray(words[:S * nb_out * 512]).view(np.uint16).reshape(S, nb_out, 2, 64, 8)
    head, tail, seen = into
    for s in range(S):
        for mb in range(nb_out):
            for lane in range(64):
                r, g = lane & 15, lane >> 4
                for j in range(8):
                    row, c = 16 * mb + r, col(s, g, j)
                    h, t = halves[s, mb, 0, lane, j], halves[s, mb, 1, lane, j]
                    if row < n_out and c is not None and c < n_in:
                        head[row, c], tail[row, c] = h, t
                        seen[row, c] += 1
                    else:
                        assert h == 0 and t == 0, (s, mb, lane, j)
    return S * nb_out * 512


def unpack(p, F, H, K, V, hops, with_comm):
    """The four bf16 fragment arrays -> {weight name: (head bits, tail bits)}; every weight seen exactly once, all padding zero, every
    array exactly as long as its layers."""
    nbH, nbV, nbM = nb(H), nb(V), nb(H + V)
    out = {}

    def fresh(n_out, n_in):
        return np.zeros((n_out, n_in), np.uint16), np.zeros((n_out, n_in), np.uint16), np.zeros((n_out, n_in), np.int64)

    def layer(name, words, nbo, sources, n_out, n_in):
        acc = fresh(n_out, n_in)
        for src in sources:
            words = words[unpack_fragment(words, nbo, src, n_out, n_in, acc):]
        assert (acc[2] == 1).all(), name
        out[name] = acc[:2]
        return words

    for arr in (p["frag_encode"], p["frag_proj"], p["frag_msg"], p["frag_head"]):
        assert arr is None or (arr.dtype == np.uint32 and arr.ndim == 1)
    rest = layer("obs2hidden.0.weight", p["frag_encode"], nbH, [rows(F, 0)], H, F)
    rest = layer("obs2hidden.2.weight", rest, nbH, [regs(nbH)], H, H)
    assert rest.size == 0
    if with_comm:
        rest = p["frag_proj"]
        for n in ("query", "key", "value"):
            rest = layer("comm.hidden2%s.0.weight" % n, rest, nbH, [regs(nbH)], H, H)
        for n, dim, nbo in (("query", K, 1), ("key", K, 1), ("value", V, nbV)):
            rest = layer("comm.hidden2%s.2.weight" % n, rest, nbo, [regs(nbH)], dim, H)
        assert rest.size == 0
        if hops > 1:
            M = H + V      # the comm columns [0, V) of [comm, h], then - in k-steps of their own - the h columns
            rest = layer("comm.msg_state2state.0.weight", p["frag_msg"], nbM, [rows(V, 0), rows(H, V)], M, M)
            rest = layer("comm.msg_state2state.2.weight", rest, nbH, [regs(nbM)], H, M)
            assert rest.size == 0
        else:
            assert p["frag_msg"] is None
        rest = layer("comm_hidden2action.0.weight", p["frag_head"], nbH, [rows(H + V, 0)], H, H + V)
    else:
        assert p["frag_proj"] is None and p["frag_msg"] is None
        rest = layer("hidden2action.0.weight", p["frag_head"], nbH, [rows(H, 0)], H, H)
    assert rest.size == 0
    return out


# ---- the synthetic inputs of the GPU tests
def make_actor(F, H=64, K=8, V=16, c=10, hops=1, seed=11, **kw):
    """As tests/test_gpu_tarmac_fused.py::_actor, on the CPU: torch's default init with the weights doubled, a fixed seed.  (With
    undoubled weights a forward that drops a cross term stays inside the contract: such an actor could not tell the kernels apart.)"""
    import torch
    from mdr_amd.tarmac import TarMACActor
    torch.manual_seed(seed)
    actor = TarMACActor(F, num_key=K, num_value=V, hidden_state_size=H, number_agents_comm=c, num_hops=hops, **kw)
    with torch.no_grad():
        for name, p in actor.named_parameters():
            if name.endswith("weight"):
                p.mul_(2.0)
    return actor


def state_dict(actor):
    return {k: v.detach().cpu().numpy() for k, v in actor.state_dict().items()}


def make_obs(E, N, F, seed=0):
    import torch
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return torch.randn((E, N, F), generator=g)


# (E, N): one agent; A = 15; one 16-agent column block; one whole 32-agent tile; a tile and one agent; A = 77, tiles that span envs;
# several attention tiles per env
CORNERS = [(1, 1), (3, 5), (1, 16), (1, 32), (1, 33), (7, 11), (2, 300)]
CORNER_HOPS = {(7, 11): (1, 2, 4), (2, 300): (1, 2, 4)}
# The observations are drawn with seed 1000 + hops, except for the single agent: one agent has one logit, and whether a dropped
# cross term moves it past the contract is chance (of the seeds 1..16 five tell the forward without Wl.xh apart, six the one without
# Wh.xl, seven the heads-only one).  Seed 16 is the first on which the fp64 reference tells all three wrong forms apart - found with
# the CPU emulation above alone, never with a kernel.
CORNER_OBS_SEED = {(1, 1): 16}
OTHER_BLOCKS = [(64, 48, 16, 32), (3, 64, 4, 4)]      # (F, H, K, V): the general form; an odd half k-step (H + V = 80 has it too)
DEFECTS = dict(E=5, N=50, hops=2, prob=0.3, seed=77, step=12)


def synthetic_inputs():
    """name -> dict(actor kwargs `kw`, E, N, F, obs seed `obs_seed`, and for the defect case `defects`): every synthetic input of the GPU
    file except the grid-stride one, whose size follows the device (grid_stride_input)."""
    out = {}
    for E, N in CORNERS:
        for hops in CORNER_HOPS.get((E, N), (1,)):
            out["E%d N%d hops%d" % (E, N, hops)] = dict(kw=dict(F=51, hops=hops), E=E, N=N, obs_seed=CORNER_OBS_SEED.get((E, N), hops))
    for F, H, K, V in OTHER_BLOCKS:
        for hops in (1, 2):
            out["F%d H%d K%d V%d hops%d" % (F, H, K, V, hops)] = dict(kw=dict(F=F, H=H, K=K, V=V, hops=hops), E=7, N=11, obs_seed=0)
    out["with_comm=False"] = dict(kw=dict(F=51, with_comm=False), E=7, N=11, obs_seed=0)
    out["comm_mode=none"] = dict(kw=dict(F=51, comm_mode="none"), E=7, N=11, obs_seed=0)
    d = DEFECTS
    out["defects"] = dict(kw=dict(F=51, hops=d["hops"], comm_defect_prob=d["prob"]), E=d["E"], N=d["N"], obs_seed=0, defects=True)
    return out


def build_input(spec):
    """-> (actor on the CPU, obs float32 tensor [E, N, F], fp64 reference probabilities [E, N, 2], the reference's keyword arguments)."""
    actor = make_actor(**spec["kw"])
    obs = make_obs(spec["E"], spec["N"], spec["kw"]["F"], spec["obs_seed"])
    ref_kw = reference_kwargs(actor, spec)
    return actor, obs, tr.actor_forward(state_dict(actor), obs.numpy(), 10, actor.num_hops, **ref_kw), ref_kw


def reference_kwargs(actor, spec):
    kw = dict(with_comm=actor.with_comm, mode=tr.NONE if actor.comm_mode == "none" else tr.NEIGHBOURS)
    if spec.get("defects"):
        d = DEFECTS
        kw["dead"] = [tr.dead_mask(d["E"], d["N"], d["prob"], d["seed"], d["step"], hop=h) for h in range(d["hops"])]
    return kw


GRID_N, GRID_HOPS, AGENTS_PER_WAVE, WAVES_PER_WORKGROUP = 50, 2, 32, 8


def grid_stride_input(cus):
    """The launcher's grid rule (csrc/mdr_tarmac_mlp_bf16.hip): min(ceil(tiles / 8), CUs) workgroups of 8 waves, 32 agents per wave and
    tile - one pass of the grid covers CUs * 256 agents.  E is chosen so that A = 50 E is two full passes plus a partial third: every
    wavefront takes at least two tiles, some three.  -> (E, per_pass, the envs the fp64 reference is held to: the first, the last, and
    those on either side of each pass boundary)."""
    per_pass = cus * WAVES_PER_WORKGROUP * AGENTS_PER_WAVE
    E = (2 * per_pass + per_pass // 16) // GRID_N + 1
    assert 2 * per_pass < E * GRID_N < 3 * per_pass
    envs = sorted({0, E - 1, *(b // GRID_N + d for b in (per_pass, 2 * per_pass) for d in (-1, 0, 1))})
    return E, per_pass, envs


def grid_stride_obs(E, device="cpu"):
    import torch
    g = torch.Generator(device="cpu").manual_seed(3)
    return torch.randn((E, GRID_N, 51), generator=g).to(device)
