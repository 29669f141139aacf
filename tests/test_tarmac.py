"""TarMAC-PPO actor on the CPU: the recorded reference cases against the dense torch path and against tests/tarmac_ref.py, the
banded restatement against the dense masked form, and the attention bound against deliberately wrong bands.  No GPU."""
import numpy as np
import pytest
import torch

from tests import actor_ref as ar
from tests import tarmac_ref as tr

CASES = tr.load_cases()
NAMES = sorted(CASES)


@pytest.mark.parametrize("name", NAMES)
def test_reference_state_dict_loads_strictly(name):
    case = CASES[name]
    actor = tr.make_actor(case)      # load_state_dict(strict=True) inside
    assert set(actor.state_dict()) == set(case["sd"])
    for k, w in actor.state_dict().items():
        assert tuple(w.shape) == case["sd"][k].shape and w.dtype == torch.float32


@pytest.mark.parametrize("name", NAMES)
def test_dense_forward_reproduces_the_fixture(name):
    case = CASES[name]
    actor = tr.make_actor(case)
    obs = torch.from_numpy(case["obs"])
    with torch.no_grad():
        p64 = actor.double()(obs.double()).numpy()
        p32 = actor.float()(obs).numpy()
    assert p64.shape == case["probs"].shape
    assert np.abs(p64 - case["probs"]).max() <= 1e-12
    assert p32.dtype == np.float32
    ratio = ar.contract_ratio(p32, case["probs"], False)
    print("%s: fp32 dense forward at %.3f of the probability contract" % (name, ratio.max()))
    assert ratio.max() <= 1.0


@pytest.mark.parametrize("name", NAMES)
def test_banded_restatement_equals_dense_and_fixture(name):
    case = CASES[name]
    kw = dict(nb_comm=case["c"], num_hops=case["hops"], mode=case["mode"], with_comm=case["with_comm"])
    band = tr.actor_forward(case["sd"], case["obs"], **kw)
    dense = tr.actor_forward(case["sd"], case["obs"], dense=True, **kw)
    assert np.abs(band - dense).max() <= 1e-12
    assert np.abs(band - case["probs"]).max() <= 1e-12


def test_offsets_and_mask_row():
    assert tr.offsets(3) == [1, -1, 2] and tr.offsets(4) == [1, -1, 2, -2]
    assert tr.band_mask(6, 3)[0].astype(int).tolist() == [1, 1, 1, 0, 0, 1]      # the issue's example row
    assert not tr.band_mask(6, 3, tr.NONE).any()
    assert tr.band_mask(4, 10).all()                                             # c >= N clamps to every other agent
    assert np.array_equal(tr.band_mask(5, 0), np.eye(5, dtype=bool))


@pytest.mark.parametrize("N,c,mode", [(6, 3, tr.NEIGHBOURS), (7, 5, tr.NEIGHBOURS), (4, 10, tr.NEIGHBOURS), (2, 10, tr.NEIGHBOURS),
                                      (1, 10, tr.NEIGHBOURS), (9, 0, tr.NEIGHBOURS), (20, 10, tr.NEIGHBOURS), (9, 4, tr.NONE)])
@pytest.mark.parametrize("defects", [False, True])
def test_band_attention_equals_dense_attention(N, c, mode, defects):
    q, k, v = tr.comm_inputs(3, N, 8, 16, seed=5)
    dead = tr.dead_mask(3, N, 0.4, seed=9, step=3) if defects else None
    band, _ = tr.band_attention(q, k, v, c, mode, dead)
    dense = tr.dense_attention(q, k, v, c, mode, dead)
    assert np.abs(band - dense).max() <= 1e-12
    if mode == tr.NONE:
        assert not band.any()
    if c == 0 or N == 1:
        assert np.array_equal(band, v.astype(np.float64))


def test_dense_torch_path_takes_the_dead_mask():
    case = CASES["f51_n50_c10_hops2"]
    dead = [tr.dead_mask(4, case["N"], 0.3, seed=11, step=2, hop=h) for h in range(case["hops"])]
    assert 0.15 < np.mean(dead) < 0.45 and not np.array_equal(dead[0], dead[1])
    ref = tr.actor_forward(case["sd"], case["obs"], case["c"], case["hops"], dead=dead)
    actor = tr.make_actor(case, defect_prob=0.3).double()
    with torch.no_grad():
        with pytest.raises(ValueError):
            actor(torch.from_numpy(case["obs"]).double())      # the dense path never draws: the mask is explicit
        p = actor(torch.from_numpy(case["obs"]).double(), dead=torch.from_numpy(np.stack(dead))).numpy()
    assert np.abs(p - ref).max() <= 1e-12
    assert np.abs(ref - case["probs"]).max() > 1e-3            # and the defects matter


def test_defect_draws_are_a_stream_of_their_own():
    u = tr.dead_uniform(3, 20, seed=7, step=5)
    assert u.dtype == np.float32 and u.shape == (3, 20) and 0 < u.min() and u.max() < 1
    assert not np.array_equal(u, ar.draw_u(np.arange(60), 7, 5).reshape(3, 20))                     # not the action stream
    assert np.array_equal(tr.dead_uniform(3, 20, 7, 5, step_dev=4), tr.dead_uniform(3, 20, 7, 9))    # step_dev adds to the low word
    assert not np.array_equal(u, tr.dead_uniform(3, 20, 7, 5, hop=1))
    assert not tr.dead_mask(3, 20, 0.0, 7, 5).any() and tr.dead_mask(3, 20, 1.0, 7, 5).all()


def test_unsupported_configurations_are_refused():
    from mdr_amd.tarmac import TarMACActor, TarMACCritic
    for kw in (dict(comm_mode="all"), dict(comm_mode="random_sample"), dict(with_gru=True), dict(num_hops=5),
               dict(attention="band", num_key=6), dict(attention="band", num_value=68), dict(attention="band", num_key=36)):
        with pytest.raises(ValueError):
            TarMACActor(22, **kw)
    actor = TarMACActor(22, attention="band")
    with pytest.raises(ValueError):
        actor(torch.zeros(2, 5, 22))                        # band: CUDA only
    with pytest.raises(ValueError):
        TarMACActor(22)(torch.zeros(10, 22))                # [E, N, F], not rows
    prop = {"actor_hidden_state_size": 32, "critic_hidden_layer_size": 64, "communication_size": 8, "key_size": 4, "comm_num_hops": 2,
            "with_gru": False, "with_comm": True, "number_agents_comm_tarmac": 6, "tarmac_comm_mode": "neighbours", "tarmac_comm_defect_prob": 0.1}
    a = TarMACActor.from_config(prop, 22)
    assert (a.hidden, a.num_value, a.num_key, a.num_hops, a.number_agents_comm, a.comm_defect_prob) == (32, 8, 4, 2, 6, 0.1)
    assert TarMACCritic(5, 22)(torch.zeros(3, 5, 22)).shape == (3, 5)


def _agents_outside(comm, ref, bound):
    return (np.abs(comm.astype(np.float64) - ref) > bound).any(axis=2)


@pytest.mark.parametrize("shape", tr.COMM_CASES + [s + ("defects",) for s in tr.DEFECT_CASES], ids=str)
def test_the_yardstick_discriminates(shape):
    """A float32 numpy evaluation of the banded formula stays inside bound_comm on every GPU-test input; the three wrong bands leave
    it for more than half of the agents on the same inputs."""
    E, N, c, K, V = shape[:5]
    q, k, v = tr.comm_inputs(E, N, K, V)
    dead = tr.dead_mask(E, N, 0.3, seed=21, step=4) if len(shape) > 5 else None
    ref, bound = tr.band_attention(q, k, v, c, dead=dead)
    got, _ = tr.band_attention(q, k, v, c, dead=dead, dtype=np.float32)
    assert got.dtype == np.float32
    assert not _agents_outside(got, ref, bound).any()
    cc = tr.clamp(c, N)
    wrong = []
    if cc >= 1:
        wrong += [("no 1/sqrt(K)", dict(scale=False)), ("no self term", dict(with_self=False))]
    if cc % 2 == 1 and cc < N - 1:      # with every other agent in the band the signs do not matter
        wrong.append(("offset signs swapped", dict(swapped=True)))
    for what, kw in wrong:
        bad, _ = tr.band_attention(q, k, v, c, dead=dead, **kw)
        frac = _agents_outside(bad, ref, bound).mean()
        assert frac > 0.5, (what, frac)
