"""CPU: the restatement of the comm modes "all" and "random_sample" (tests/tarmac_gather_ref.py) held to account - the Floyd / Philox
draw, the gather form against its dense twin, the dense torch path with ``mask=`` against the reference's recorded probabilities, the
rounding bound (kept by float32, left by three wrong variants) - and the constructor rules of ``TarMACActor``."""
import numpy as np
import pytest
import torch

from tests import tarmac_gather_ref as gr
from tests import tarmac_ref as tr
from tests.actor_ref import draw_word, uniform_of

SEED, STEP = gr.SEED, gr.STEP


@pytest.mark.parametrize("N", [1, 2, 5, 20, 300])
@pytest.mark.parametrize("c", [0, 1, 3, 10, 64])
def test_every_set_is_self_plus_c_distinct_others(N, c):
    E = 3
    idx = gr.sample_index(E, N, c, SEED, STEP)
    cc = min(c, N - 1)
    assert idx.shape == (E, N, cc + 1) and idx.dtype == np.int64
    assert np.array_equal(idx[:, :, 0], np.broadcast_to(np.arange(N), (E, N)))
    assert idx.min() >= 0 and idx.max() < N
    s = np.sort(idx, axis=2)
    assert (np.diff(s, axis=2) > 0).all()                                # distinct, hence c others besides self
    assert gr.mask_of(idx, N).sum(axis=2).min() == cc + 1


@pytest.mark.parametrize("N", [2, 5, 20, 65])
def test_full_sample_is_the_full_set(N):
    idx = gr.sample_index(2, N, N - 1, SEED, STEP)
    assert gr.mask_of(idx, N).all()
    assert np.array_equal(gr.sample_index(2, N, 1000, SEED, STEP), idx)  # the clamp


def test_step_dev_adds_to_the_low_word():
    a = gr.sample_index(4, 20, 10, SEED, 5, step_dev=4)
    assert np.array_equal(a, gr.sample_index(4, 20, 10, SEED, 9))
    wrap = gr.sample_index(4, 20, 10, SEED, (3 << 32) + 0xFFFFFFFE, step_dev=7)
    assert np.array_equal(wrap, gr.sample_index(4, 20, 10, SEED, (3 << 32) + 5))      # no carry into the high word
    assert not np.array_equal(wrap, gr.sample_index(4, 20, 10, SEED, (4 << 32) + 5))


def test_hop_seed_step_and_env_change_the_draw():
    base = gr.sample_index(4, 20, 10, SEED, STEP)
    assert not np.array_equal(base, gr.sample_index(4, 20, 10, SEED, STEP, hop=1))
    assert not np.array_equal(base, gr.sample_index(4, 20, 10, SEED + 1, STEP))
    assert not np.array_equal(base, gr.sample_index(4, 20, 10, SEED, STEP + 1))
    assert not np.array_equal(base[0], base[1]) and not np.array_equal(base[1], base[2])
    # independent of the env count: env e of a larger batch draws what it draws in a smaller one
    assert np.array_equal(gr.sample_index(7, 20, 10, SEED, STEP)[:4], base)


def test_the_stream_is_not_the_action_or_the_dead_sender_stream():
    agent = np.arange(4096, dtype=np.uint64)
    for hop in range(4):
        for j in (0, 1, 2, 3, 4, 18):
            w = gr.sample_word(agent, j, SEED, STEP, 0, hop).astype(np.uint32)
            assert not (w == draw_word(agent, SEED, STEP)).any()
            dead = tr.dead_uniform(4096 // 16, 16, SEED, STEP, 0, hop).reshape(-1)      # the same agents, 24 bits of their words
            assert (uniform_of(w) == dead).mean() < 1e-3
    # structurally: bit 31 of the second counter word is set here and never there (agent indices below 2^48)
    assert gr.TAG_GATHER not in (tr.TAG_TARMAC, 0x41435431)


def test_every_other_agent_is_chosen_with_frequency_c_over_m():
    E, N, c = 4096, 20, 10
    mask = gr.mask_of(gr.sample_index(E, N, c, SEED, STEP), N)
    count = mask.sum(axis=0).astype(np.float64)                          # [receiver, sender]
    off = ~np.eye(N, dtype=bool)
    p = c / (N - 1)
    sd = np.sqrt(E * p * (1 - p))
    assert np.abs(count[off] - E * p).max() <= 5 * sd
    assert (count[~off] == E).all()


@pytest.mark.parametrize("mode", [gr.ALL, gr.RANDOM_SAMPLE])
@pytest.mark.parametrize("shape", [s for s in gr.GATHER_CASES if s[1] <= 65], ids=str)
def test_gather_form_equals_its_dense_twin(shape, mode):
    ref = gr.reference(shape, mode)
    got = gr.gather_attention(ref["q"], ref["k"], ref["v"], ref["idx"])
    np.testing.assert_allclose(got, ref["out"], rtol=0, atol=1e-12)
    if shape[1] == 1 or shape[2] == 0:
        assert np.array_equal(got.astype(np.float32), ref["v"])


@pytest.mark.parametrize("mode", [gr.ALL, gr.RANDOM_SAMPLE])
@pytest.mark.parametrize("shape", gr.GATHER_CASES, ids=str)
def test_float32_restatement_stays_inside_the_bound(shape, mode):
    ref = gr.reference(shape, mode)
    got = gr.gather_attention(ref["q"], ref["k"], ref["v"], ref["idx"], dtype=np.float32)
    assert got.dtype == np.float32
    assert gr.worst(got, ref["out"], ref["bound"]) <= 1.0


@pytest.mark.parametrize("mode", [gr.ALL, gr.RANDOM_SAMPLE])
def test_wrong_variants_leave_the_bound(mode):
    shape = (13, 20, 10, 8, 16)
    ref = gr.reference(shape, mode)
    q, k, v, idx = ref["q"], ref["k"], ref["v"], ref["idx"]
    N = shape[1]
    own = idx == np.arange(N)[None, :, None]
    no_self = idx[~own].reshape(idx.shape[0], N, idx.shape[2] - 1)
    doubled = np.concatenate([idx, idx[:, :, -1:]], axis=2)
    for wrong in (gr.gather_attention(q, k, v, no_self, dtype=np.float32), gr.gather_attention(q, k, v, doubled, dtype=np.float32),
                  gr.gather_attention(q, k, v, idx, dtype=np.float32, scale=False)):
        assert gr.worst(wrong, ref["out"], ref["bound"]) > 1.0


@pytest.mark.parametrize("mode", [gr.ALL, gr.RANDOM_SAMPLE])
def test_gradient_restatement_and_its_bound(mode):
    """The closed form against central differences of the dense attention; float32 autograd of the same formula inside the bound."""
    shape = (4, 2, 10, 8, 16) if mode == gr.ALL else (13, 20, 10, 8, 16)
    ref = gr.reference(shape, mode)
    q, k, v, g, mask = (ref[n] for n in ("q", "k", "v", "g", "mask"))
    dq, dk, dv = ref["grad"]
    h = 1e-6
    for arr, grad, which in ((q, dq, 0), (k, dk, 1), (v, dv, 2)):
        for pos in ((0, 0, 0), (1, shape[1] - 1, 3)):
            ops = [np.asarray(t, dtype=np.float64).copy() for t in (q, k, v)]
            ops[which][pos] += h
            up = (gr.dense_attention(*ops, mask) * g).sum()
            ops[which][pos] -= 2 * h
            dn = (gr.dense_attention(*ops, mask) * g).sum()
            assert abs((up - dn) / (2 * h) - grad[pos]) <= 1e-6 * max(1.0, abs(grad[pos]))
    tq, tk, tv = (torch.tensor(t, requires_grad=True) for t in (q, k, v))
    s = torch.matmul(tq, tk.transpose(-2, -1)) / np.float32(np.sqrt(shape[3]))
    s = s.masked_fill(~torch.tensor(mask), -float("inf"))
    (torch.softmax(s, dim=-1) @ tv * torch.tensor(g)).sum().backward()
    for got, want, bound in zip((tq.grad, tk.grad, tv.grad), ref["grad"], ref["grad_bound"]):
        assert gr.worst(got.numpy(), want, bound) <= 1.0


CASES = gr.load_cases()


def _case_masks(case):
    m = torch.from_numpy(case["masks"])
    return m if case["mode"] == gr.RANDOM_SAMPLE else None


@pytest.mark.parametrize("name", sorted(CASES))
def test_dense_path_with_masks_reproduces_the_reference(name):
    case = CASES[name]
    assert case["masks"].shape == (case["hops"], case["N"], case["N"])
    assert (case["masks"].sum(axis=2) == (case["N"] if case["mode"] == gr.ALL else min(case["c"], case["N"] - 1) + 1)).all()
    actor = gr.make_actor(case, "dense", torch.float64)
    obs = torch.from_numpy(case["obs"]).double()
    with torch.no_grad():
        for mask in (torch.from_numpy(case["masks"]), _case_masks(case)):
            if mask is None and case["mode"] == gr.RANDOM_SAMPLE:
                continue
            np.testing.assert_allclose(actor(obs, mask=mask).numpy(), case["probs"], rtol=0, atol=1e-12)
        # one mask per env, [hops, E, N, N], is the same thing
        per_env = torch.from_numpy(case["masks"])[:, None].expand(-1, obs.shape[0], -1, -1)
        np.testing.assert_allclose(actor(obs, mask=per_env).numpy(), case["probs"], rtol=0, atol=1e-12)
    if case["mode"] == gr.RANDOM_SAMPLE:
        with pytest.raises(ValueError):
            actor(obs)                                                   # no fixed mask: mask= is required
        with pytest.raises(ValueError):
            actor(obs, mask=torch.ones((case["hops"] + 1, case["N"], case["N"]), dtype=torch.bool))


def test_constructor_rules():
    from mdr_amd.tarmac import GATHER_MODES, MODES, TarMACActor
    assert MODES == {"neighbours": 0, "none": 1} and GATHER_MODES == {"all": 0, "random_sample": 1}
    for mode in ("all", "random_sample"):
        with pytest.raises(ValueError):
            TarMACActor(22, comm_mode=mode)                              # attention="auto": refused as before
        with pytest.raises(ValueError):
            TarMACActor(22, comm_mode=mode, attention="band")
        for attention in ("gather", "dense"):
            a = TarMACActor(22, comm_mode=mode, attention=attention)
            assert a.comm_mode == mode and a.attention == attention
    for mode in ("neighbours", "none"):
        with pytest.raises(ValueError):
            TarMACActor(22, comm_mode=mode, attention="gather")
    with pytest.raises(ValueError):
        TarMACActor(22, comm_mode="all", attention="gather", num_key=6)  # the kernels' row limits, checked at construction
    prop = dict(key_size=8, communication_size=16, actor_hidden_state_size=8, number_agents_comm_tarmac=10, tarmac_comm_mode="random_sample",
                comm_num_hops=1, with_comm=True)
    with pytest.raises(ValueError):
        TarMACActor.from_config(prop, 22)
    assert TarMACActor.from_config(prop, 22, attention="gather").attention == "gather"
    # gather runs on the GPU only
    actor = TarMACActor(22, comm_mode="all", attention="gather", hidden_state_size=8)
    with pytest.raises(ValueError):
        actor(torch.zeros((1, 3, 22)))
    with pytest.raises(ValueError):
        actor.sample(torch.zeros((1, 3, 22)), 0, 0)


def test_fused_actor_and_update_kernels_keep_refusing():
    from mdr_amd import tarmac_ppo
    from mdr_amd.tarmac import FusedTarMACActor, TarMACActor
    for mode in ("all", "random_sample"):
        actor = TarMACActor(22, comm_mode=mode, attention="gather", hidden_state_size=8)
        with pytest.raises(ValueError):
            FusedTarMACActor.from_module(actor)
        assert not tarmac_ppo.supported(actor)
        assert tarmac_ppo._refusal(actor) == "the kernels cover the comm modes 'neighbours' and 'none'"
