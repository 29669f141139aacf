"""Every instantiation of the fused actor kernels (csrc/mdr_policy.hip: 13 on observation rows, 74 observe -> act) against a plain
fp64 forward of the same network and against the restated Philox draw (tests/actor_ref.py), one case per form.

CASES names the form each case is for; tests/actor_forms.py restates the selection that leads to it and
tests/test_actor_forms.py (no GPU) fails when a reachable form has no case here.  Shapes sit on the edge that selects the form
(62 features: the last count the 32-register form of k_actor_sample takes; 112 / 113 hidden units: seven or eight 16-row blocks;
64 / 65 features: 16 or 32 feature registers), batches end in a partial tile wherever the cluster size allows one.

Per case: probabilities within the project's contract of the fp64 forward (fp32 layouts 1e-5 |p| + 2e-6; bf16x3 2e-3 |p| + 2e-5 and
mean |error| < 5e-6); the logit difference log(p0 / p1) within the derived running bound + 8 ulp of the fp64 one wherever both
probabilities are normal numbers; the action of EVERY agent equal to the restated draw on the kernel's own p0; a_prob the bits of
probs[action]; greedy = the sign of the kernel's own logit difference, and the fp64 argmax wherever that is clear of the bound.
Each case prints its worst figures (profiles/actor_forms_README.md records them)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import actor_forms as af
from tests import actor_ref as ar

pytestmark = pytest.mark.gpu

ALL_FLAGS = ("hour", "day", "solar_gain", "thermal", "hvac")
# observation shapes of the extended observe -> act forms by their compile-time k-steps of layer 1: 51, 58 and 63 features
SHAPES = {0: dict(flags=(), defects=0.0),                       # the default observation: not extended
          13: dict(flags=(), defects=0.1),                      # the default columns with link defects
          15: dict(flags=("thermal", "hvac"), defects=0.0),
          16: dict(flags=ALL_FLAGS, defects=0.0)}
GRID_AGENTS = 5 * 65536 + 3 * 16 + 5      # 256 CUs x 8 (16) waves x 32 (16) agents fill the grid once: five passes and a partial tile


def _rows_case(form, layout, F, layers):
    return dict(form=form, kind="rows", layout=layout, F=F, layers=layers)


def _observe_case(layout, layers, N, extk, store, table=False):
    shape = SHAPES[extk]
    ext, c, own = af.observe_shape(shape["flags"], 10, shape["defects"], table)
    form, waves = af.select_observe(layout, layers[0], layers[1], N, 37, ext, c, own, table, store)
    return dict(form=form, kind="observe", layout=layout, layers=layers, N=N, E=37 if N % 32 else 29, extk=extk, store=store, table=table,
                waves=waves)


CASES = [
    _rows_case("k_actor_sample<32,52>", 0, 62, (100, 100)),
    _rows_case("k_actor_sample<32,0>", 0, 51, (64, 32)),
    _rows_case("k_actor_sample<0,0>", 0, 133, (127, 127)),
    _rows_case("k_actor_sample16<7,false,16>", 1, 64, (112, 112)),
    _rows_case("k_actor_sample16<8,false,16>", 1, 11, (113, 64)),
    _rows_case("k_actor_sample16<7,true,16>", 3, 51, (100, 100)),
    _rows_case("k_actor_sample16<7,false,32>", 1, 65, (64, 100)),
    _rows_case("k_actor_sample16<8,false,32>", 1, 128, (127, 127)),
    _rows_case("k_actor_sample16<7,true,32>", 3, 128, (97, 99)),
    _rows_case("k_actor_sample_bf16<7,16>", 2, 64, (100, 100)),
    _rows_case("k_actor_sample_bf16<8,16>", 2, 33, (113, 64)),
    _rows_case("k_actor_sample_bf16<7,32>", 2, 65, (112, 100)),
    _rows_case("k_actor_sample_bf16<8,32>", 2, 128, (127, 127)),
]
# the default observation: lean staging (64 houses per env) and the general one (50), with and without the rows written on the side
CASES += [_observe_case(layout, layers, N, 0, store)
          for layout, layers in ((1, (100, 100)), (1, (127, 120)), (3, (100, 100)), (2, (100, 100)), (2, (127, 127)))
          for N in (64, 50) for store in (True, False)]
# extended fp32 forms, circular neighbours: the 4x4-tail actor keeps a whole-tile staging for N % 32 == 0, the others take the windows
CASES += [_observe_case(3, (100, 100), N, extk, store) for N in (64, 50) for extk in (13, 15, 16) for store in (True, False)]
CASES += [_observe_case(1, layers, 50, extk, store) for layers in ((100, 100), (127, 127)) for extk in (13, 15, 16) for store in (True, False)]
# ... and senders through a link table (closed groups)
CASES += [_observe_case(layout, layers, 50, extk, store, table=True) for layout, layers in ((3, (100, 100)), (1, (100, 100)), (1, (127, 127)))
          for extk in (13, 15, 16) for store in (True, False)]
# extended bf16x3 forms: seven blocks on 51 features, eight on 63 (six or seven windows beside the fragments instead of eight)
CASES += [_observe_case(2, layers, N, extk, store, table) for layers, extk in (((100, 100), 13), ((127, 127), 16))
          for N, table in ((64, False), (50, False), (50, True)) for store in (True, False)]


def _case_id(case):
    return case["form"]


# ---- helpers ------------------------------------------------------------------------------------------------------------------

def _module(F, layers, seed, scale, keep=None):
    return ar.make_actor(F, layers, seed, scale, keep).to("cuda:0")


def _saturated_module(F, layers=(100, 100)):
    """Zero weights and a head bias difference of +200: p0 == 1.0f and p1 == 0.0f for every agent."""
    actor = _module(F, layers, 0, 0.0)
    with torch.no_grad():
        for lin in actor.fc:
            lin.bias.zero_()
        actor.fc[2].bias.copy_(torch.tensor([200.0, 0.0]))
    return actor


def rows_inputs(F, A, seed):
    return ar.rows_inputs(F, A, seed).to("cuda:0")


@functools.lru_cache(maxsize=None)
def _env(N, E, extk, table):
    import mdr_amd
    from tests.test_gpu_observe_act import _shape_cfg, _walk
    shape = SHAPES[extk]
    cfg = _shape_cfg(N, shape["flags"], 10, shape["defects"])
    if table:
        cfg["default_env_prop"]["cluster_prop"]["agents_comm_mode"] = "closed_groups"
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=5 + N)
    env.reset(episode=1)
    _walk(env, 7, seed=extk)
    return env


def check_outputs(tag, layout, weights, rows, action, a_prob, probs, greedy_action, seed, step, step_dev=0, agents=None, ref=None,
                  cap=True):
    """Everything the module docstring promises for one launch; `rows`, the outputs and `agents` (indices in the whole batch,
    default 0 .. A - 1) as numpy arrays on the CPU; `ref`: a torch fp32 forward of the module on the same rows, only printed - how
    far an fp32 forward that is not the kernel sits from fp64 on these inputs, in units of the fp32 contract.  `cap`: hold the share
    of agents whose fp64 logit difference lies inside the bound to 1 % (the networks built for it: NETWORKS)."""
    bf16 = layout == ar.BF16X3
    A = rows.shape[0]
    agents = np.arange(A, dtype=np.uint64) if agents is None else np.asarray(agents, dtype=np.uint64)
    d64, p0, p1, bound = ar.forward64(*weights, rows, layout=layout)
    ratio = np.maximum(ar.contract_ratio(probs[:, 0], p0, bf16), ar.contract_ratio(probs[:, 1], p1, bf16))
    dk, normal = ar.kernel_logit_difference(probs)
    limit = bound + 8.0 * ar.ulp32(d64)
    dratio = np.abs(dk[normal] - d64[normal]) / limit[normal]
    mean_abs = float(np.abs(probs.astype(np.float64) - np.stack([p0, p1], 1)).mean())
    clear = np.abs(d64) > limit
    torch_ratio = -1.0 if ref is None else float(np.maximum(ar.contract_ratio(ref[:, 0], p0, False), ar.contract_ratio(ref[:, 1], p1, False)).max())
    print("ACTOR_FORM %s agents=%d contract=%.4f dbound=%.5f mean_abs=%.3e normal=%.3f unclear=%.5f torch_fp32=%.4f"
          % (tag, A, ratio.max(), dratio.max() if dratio.size else -1.0, mean_abs, normal.mean(), 1.0 - clear.mean(), torch_ratio))
    assert np.isfinite(probs).all()
    worst = int(ratio.argmax())
    assert ratio.max() <= 1.0, "%s: agent %d probs %r against fp64 (%r, %r)" % (tag, worst, probs[worst], p0[worst], p1[worst])
    if bf16:
        assert mean_abs < ar.BF16_MEAN_ABS
    assert normal.any() and dratio.max() <= 1.0, "%s: logit difference off by %.3f of its bound" % (tag, dratio.max())
    u = ar.draw_u(agents, seed, step, step_dev)
    want = ar.expected_action(u, probs[:, 0], False, None)
    wrong = np.nonzero(action != want)[0]
    assert wrong.size == 0, "%s: %d of %d actions are not the restated draw, first at %s" % (tag, wrong.size, A, wrong[:5])
    assert np.array_equal(a_prob.view(np.uint32), probs[np.arange(A), action].view(np.uint32))
    assert np.abs(probs.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
    if greedy_action is not None:
        assert np.array_equal(greedy_action, ar.expected_action(None, None, True, dk))
        assert np.array_equal(greedy_action[clear], np.where(d64 >= 0, 0, 1)[clear])
        if cap:
            assert 1.0 - clear.mean() <= 0.01, "%s: %.4f of the agents lie inside the bound" % (tag, 1.0 - clear.mean())


def _np(*tensors):
    return tuple(t.cpu().numpy() for t in tensors)


# Two networks per case.  "dense": torch's default init, the network the contract was written for.  "sparse": 8 weights per hidden
# unit - the one the greedy check's 1 % cap is held on (actor_ref.make_actor says why a dense one cannot meet it); its bound is
# several times tighter against its logits, so the logit-difference check bites harder on it too.
NETWORKS = (("dense", None, False), ("sparse", ar.SPARSE_KEEP, True))
ROWS_SCALE, OBSERVE_SCALE = 2.5, 2.0


def _run_rows(case, seed, step, step_dev=None, batches=(37, GRID_AGENTS), networks=NETWORKS):
    from mdr_amd.policy import FusedActor
    layout, F = case["layout"], case["F"]
    sel = af.select_rows(layout, F, *case["layers"])
    assert sel[0] == case["form"]
    dev = None if step_dev is None else torch.tensor([step_dev], dtype=torch.int32, device="cuda:0")
    for net, keep, cap in networks:
        actor = _module(F, case["layers"], seed=F, scale=ROWS_SCALE, keep=keep)
        weights = ar.module_weights(actor)
        fused = FusedActor.from_module(actor, layout=layout)
        greedy = FusedActor.from_module(actor, layout=layout, greedy=True)
        for A in batches:
            rows = rows_inputs(F, A, seed=A)
            action, a_prob, probs = fused.sample(rows, seed, step, want_probs=True, step_dev=dev)
            g_action, _ = greedy.sample(rows, seed, step)
            with torch.no_grad():
                ref = actor(rows)
            check_outputs("%s rows %s A=%d waves=%d" % (case["form"], net, A, sel[1]), layout, weights,
                          *_np(rows, action, a_prob, probs, g_action), seed, step, 0 if step_dev is None else step_dev,
                          ref=ref.cpu().numpy(), cap=cap and A > 10000)
            if A < 1000:      # the same batch handed over as feature planes: the same bits
                a2, p2, probs2 = fused.sample(rows.t().contiguous(), seed, step, want_probs=True, step_dev=dev)
                assert torch.equal(a2, action) and torch.equal(p2, a_prob) and torch.equal(probs2, probs)


def _run_observe(case, seed, step, step_dev=None, networks=NETWORKS):
    from mdr_amd.policy import FEATURES_OBSERVE, FusedActor
    layout, N, E = case["layout"], case["N"], case["E"]
    env = _env(N, E, case["extk"], case["table"])
    F = env.obs_vector_length()
    shape = SHAPES[case["extk"]]
    assert F == 51 + sum(af.STATE_COLUMNS[f] for f in shape["flags"])
    ext, c, own = af.observe_shape(shape["flags"], 10, shape["defects"], case["table"])
    assert af.select_observe(layout, *case["layers"], N, E, ext, c, own, case["table"], case["store"]) == (case["form"], case["waves"])
    dev = None if step_dev is None else torch.tensor([step_dev], dtype=torch.int32, device="cuda:0")
    rows = env.obs_vector("rows").view(E * N, F)
    for net, keep, cap in networks:
        actor = _module(F, case["layers"], seed=E + F, scale=OBSERVE_SCALE, keep=keep)
        weights = ar.module_weights(actor)
        kw = dict(layout=layout, feature_order=FEATURES_OBSERVE, observe_msg_floats=40)
        fused, greedy = FusedActor.from_module(actor, **kw), FusedActor.from_module(actor, greedy=True, **kw)
        outs = {}
        for store in (case["store"], not case["store"]):      # the form of this case, then its STORE sibling
            kept = torch.full((E * N, F), float("nan"), device="cuda:0") if store else None
            outs[store] = fused.sample_env(env, seed, step, want_probs=True, step_dev=dev, rows_out=kept)
            if store:
                assert torch.equal(kept, rows), "rows_out differs from obs_vector('rows')"
        for x, y in zip(outs[True], outs[False]):
            assert torch.equal(x, y), "writing the rows on the side changed an output"
        g_action, _ = greedy.sample_env(env, seed, step, rows_out=torch.empty_like(rows) if case["store"] else None)
        action, a_prob, probs = outs[case["store"]]
        with torch.no_grad():
            ref = actor(rows)
        check_outputs("%s observe %s E=%d N=%d F=%d waves=%d" % (case["form"], net, E, N, F, case["waves"]), layout, weights,
                      *_np(rows, action, a_prob, probs, g_action), seed, step, 0 if step_dev is None else step_dev,
                      ref=ref.cpu().numpy(), cap=cap)


# ---- one case per form --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_form_against_fp64_and_its_exact_draw(case):
    (_run_rows if case["kind"] == "rows" else _run_observe)(case, seed=9, step=3)


# ---- the counter words, once per kernel family --------------------------------------------------------------------------------

BIG_SEED = 0x9E3779B97F4A7C15
FAMILY_CASES = [next(c for c in CASES if c["form"] == f) for f in (
    "k_actor_sample<32,52>", "k_actor_sample16<7,false,16>", "k_actor_sample16<7,true,16>", "k_actor_sample_bf16<7,16>",
    "k_actor_observe16<7,true,false,false,0,false>", "k_actor_observe16<7,false,true,true,13,false>",
    "k_actor_observe_bf16<7,true,true,false,false>", "k_actor_observe_bf16<8,false,true,true,true>")]


@pytest.mark.parametrize("step,step_dev", [(2 ** 32 + 5, 7), (2 ** 32 + 0xFFFFFFF0, 0x20), (5 * 2 ** 32 + 3, -2)],
                         ids=["high-word", "low-word-wraps", "negative-step-dev"])
@pytest.mark.parametrize("case", FAMILY_CASES, ids=_case_id)
def test_counter_words_of_every_kernel_family(case, step, step_dev):
    """A seed with a high word, a step beyond 32 bits, a device-side step: key = (seed lo, seed hi), counter word 2 = step lo +
    *step_dev modulo 2^32 - a sum that crosses 2^32 wraps and leaves word 3 = TAG_ACTION ^ step hi alone (include/mdr_policy.h)."""
    if case["kind"] == "rows":
        _run_rows(case, BIG_SEED, step, step_dev, batches=(4099,), networks=NETWORKS[:1])
    else:
        _run_observe(case, BIG_SEED, step, step_dev, networks=NETWORKS[:1])


def test_the_restated_draw_tells_the_counter_words_apart():
    """The restatement itself (CPU arithmetic): each word of the key and the counter changes the draws."""
    agents = np.arange(4096, dtype=np.uint64)
    base = ar.draw_word(agents, BIG_SEED, 2 ** 32 + 5, 7)
    for other in (ar.draw_word(agents, BIG_SEED & 0xFFFFFFFF, 2 ** 32 + 5, 7), ar.draw_word(agents, BIG_SEED, 5, 7),
                  ar.draw_word(agents, BIG_SEED, 2 ** 32 + 5, 8), ar.draw_word(agents + np.uint64(16), BIG_SEED, 2 ** 32 + 5, 7),
                  ar.draw_word(agents + np.uint64(2 ** 32), BIG_SEED, 2 ** 32 + 5, 7)):
        assert (other != base).mean() > 0.99
    assert np.array_equal(ar.draw_word(agents, 1, 2 ** 32 + 0xFFFFFFF0, 0x20), ar.draw_word(agents, 1, 2 ** 32 + 0x10, 0))


# ---- batches beyond 4 GiB of rows: slices of whole tiles ----------------------------------------------------------------------

SLICE_AGENTS = ((0xFFFFFFFF // 512) & ~15) + 5000      # F = 128: 8,388,592 agents fill a launch; 4.3 GB of rows in all


@pytest.mark.parametrize("layout,layers,form", [(1, (100, 100), "k_actor_sample16<7,false,32>"), (3, (100, 100), "k_actor_sample16<7,true,32>")])
def test_batches_beyond_4_gib_go_out_in_slices_with_batch_wide_draws(layout, layers, form):
    from mdr_amd.policy import FusedActor
    F, A = 128, SLICE_AGENTS
    slices = af.rows_slices(F, A)
    assert len(slices) == 2 and slices[0][1] % 16 == 0 and A * F * 4 > 2 ** 32 and af.select_rows(layout, F, *layers, A=A)[0] == form
    actor = _module(F, layers, seed=1, scale=ROWS_SCALE)
    fused = FusedActor.from_module(actor, layout=layout)
    g = torch.Generator(device="cuda:0").manual_seed(4)
    rows = torch.empty((A, F), device="cuda:0")
    for lo in range(0, A, 1 << 20):      # filled in pieces: no second buffer of that size
        rows[lo:lo + (1 << 20)].normal_(0.0, 1.5, generator=g)
    action, a_prob, probs = fused.sample(rows, 9, 3, want_probs=True)
    pick = [np.arange(first, first + min(4096, count)) for first, count in slices]
    pick += [np.arange(first + count - min(4096, count), first + count) for first, count in slices]
    pick.append(np.random.default_rng(0).integers(0, A, 65536))
    agents = np.unique(np.concatenate(pick))
    idx = torch.from_numpy(agents).to("cuda:0")
    check_outputs("%s slices A=%d" % (form, A), layout, ar.module_weights(actor),
                  *_np(rows[idx], action[idx], a_prob[idx], probs[idx]), None, 9, 3, agents=agents)
    assert bool(torch.isfinite(a_prob).all()) and bool((action <= 1).all())


def test_feature_planes_beyond_32_bit_offsets_are_refused_and_the_last_that_fit_run():
    from mdr_amd.policy import FusedActor
    F, A = 128, 1000
    limit = (2 ** 32 // 4 - A) // (F - 1)                       # the widest plane stride whose last float sits below 4 GiB
    assert ((F - 1) * limit + A) * 4 <= 0xFFFFFFFF < ((F - 1) * (limit + 1) + A) * 4
    assert af.select_rows(1, F, 100, 100, A=A, plane_stride=limit + 1) == af.UNSUPPORTED
    assert af.select_rows(1, F, 100, 100, A=A, plane_stride=limit)[0] == "k_actor_sample16<7,false,32>"
    actor = _module(F, (100, 100), seed=2, scale=ROWS_SCALE)
    fused = FusedActor.from_module(actor, layout=1)
    rows = rows_inputs(F, A, seed=3)
    a0, p0, probs0 = fused.sample(rows, 9, 3, want_probs=True)
    buf = torch.empty((F - 1) * limit + A, device="cuda:0")
    planes = buf.as_strided((F, A), (limit, 1))
    planes.copy_(rows.t())
    a1, p1, probs1 = fused.sample(planes, 9, 3, want_probs=True)
    assert torch.equal(a0, a1) and torch.equal(p0, p1) and torch.equal(probs0, probs1)
    check_outputs("k_actor_sample16<7,false,32> planes stride=%d" % limit, 1, ar.module_weights(actor), *_np(rows, a1, p1, probs1), None, 9, 3)
    # one float further apart: refused before anything is launched (the buffer is never read)
    out = torch.zeros(A, dtype=torch.uint8, device="cuda:0")
    rc = fused._lib.mdr_actor_sample(C.byref(fused._desc), C.c_void_p(buf.data_ptr()), limit + 1, A, C.c_uint64(9), C.c_uint64(3), None,
                                     C.c_void_p(out.data_ptr()), None, None, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == af.UNSUPPORTED
    # the layouts that address their features by 64-bit pointers take such planes... but this test allocates no second 4 GiB for them


# ---- the top cell of the uniform ----------------------------------------------------------------------------------------------

# The draw whose 24 bits are all ones, found with the restated Philox (about 10 s on a CPU):
#   agents = np.arange(1 << 20, dtype=np.uint64)
#   for step in range(200):
#       hit = np.nonzero(actor_ref.draw_word(agents, 11, step) >> np.uint32(8) == 0xFFFFFF)[0]
#       if hit.size: print(step, hit); break                       # -> 41 [689152]
TOP_SEED, TOP_STEP, TOP_AGENT = 11, 41, 689152


def test_the_top_cell_draw_is_what_the_search_found():
    word = ar.draw_word(np.array([TOP_AGENT], dtype=np.uint64), TOP_SEED, TOP_STEP)
    assert int(word[0]) >> 8 == 0xFFFFFF
    assert ar.uniform_of(word, clamp=False)[0] == np.float32(1.0)      # 16777215.5 ties to 2^24
    assert ar.uniform_of(word)[0] == ar.U_MAX < np.float32(1.0)


@pytest.mark.parametrize("layout", [0, 1, 2, 3])
def test_top_cell_draw_never_takes_an_action_of_probability_zero_on_rows(layout):
    from mdr_amd.policy import FusedActor
    A, F = TOP_AGENT + 4097, 11
    fused = FusedActor.from_module(_saturated_module(F), layout=layout)
    action, a_prob, probs = fused.sample(torch.zeros((A, F), device="cuda:0"), TOP_SEED, TOP_STEP, want_probs=True)
    assert float(probs[TOP_AGENT, 0]) == 1.0 and float(probs[TOP_AGENT, 1]) == 0.0
    assert int(action[TOP_AGENT]) == 0, "u == 1.0f took the action whose probability is 0"
    assert int(action.sum()) == 0 and bool((a_prob > 0).all())


@pytest.mark.parametrize("layout,extk", [(1, 0), (2, 0), (3, 0), (1, 13), (2, 13)])
def test_top_cell_draw_never_takes_an_action_of_probability_zero_observe_act(layout, extk):
    from mdr_amd.policy import FEATURES_OBSERVE, FusedActor
    N = 64
    E = TOP_AGENT // N + 3
    env = _env(N, E, extk, False)
    fused = FusedActor.from_module(_saturated_module(51), layout=layout, feature_order=FEATURES_OBSERVE)
    action, a_prob, probs = fused.sample_env(env, TOP_SEED, TOP_STEP, want_probs=True)
    assert float(probs[TOP_AGENT, 0]) == 1.0 and float(probs[TOP_AGENT, 1]) == 0.0
    assert int(action[TOP_AGENT]) == 0, "u == 1.0f took the action whose probability is 0"
    assert int(action.sum()) == 0 and bool((a_prob > 0).all())
