"""tests/ppo_grad_bf16_ref.py held to account on the CPU: the split's two constants, the grid inputs' conditions, the fp32-accumulated
restatement within the derived bound of the exact fp64 values, every wrong variant outside it, the full-mantissa inputs' conditions,
and the two entry points as the header declares and mdr_amd._native binds them.  No kernel runs here."""
import re

import numpy as np
import pytest

from mdr_amd import _native as nat
from tests import ppo_grad_bf16_ref as br
from tests import ppo_grad_ref as pr
from tests.tarmac_bf16_ref import split
from tests.test_abi import _header

HEADS = pytest.mark.parametrize("O", [2, 1], ids=["actor", "critic"])
FULL_NETS = [(51, 100, 100), (64, 128, 128), (63, 97, 113)]


def test_the_two_constants_of_the_split():
    r = np.random.default_rng(1)
    a = np.concatenate([r.standard_normal(200000) * 10.0 ** r.integers(-6, 6, 200000), 2.0 ** r.integers(-20, 20, 1000),
                        (1 + 2.0 ** -8) * 2.0 ** r.integers(-20, 20, 1000), (1 + 2.0 ** -8 + 2.0 ** -17) * 2.0 ** r.integers(-20, 20, 1000)])
    a = a.astype(np.float32)
    h, t = split(a)
    a64, h64, t64 = (v.astype(np.float64) for v in (a, h, t))
    assert (np.abs(t64) <= br.TAIL * np.abs(a64)).all()
    assert (np.abs(a64 - h64 - t64) <= br.RESID * np.abs(a64)).all()
    worst = np.max(np.abs(a64 - h64 - t64) / np.abs(a64))
    assert worst > br.RESID / 4, "the constant is not slack by more than its rounding up"


@HEADS
@pytest.mark.parametrize("net", br.NETS, ids=lambda n: "F%d-H%d-%d" % n)
def test_grid_inputs_make_the_forward_exact_and_exercise_the_tails(net, O):
    d = br.draw(*net, O)
    x, W1, b1, W2, b2 = (d[k].astype(np.float64) for k in ("x", "W1", "b1", "W2", "b2"))
    assert set(np.unique(d["x"])) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(np.round(W1 * 2048), W1 * 2048) and np.abs(W1).max() <= 0.5
    assert np.array_equal(np.round(W2 * 64), W2 * 64) and np.abs(W2).max() <= 4 / 64
    assert all(np.array_equal(np.round(d[k] * 32.0), d[k] * 32.0) and np.abs(d[k]).max() <= 0.25 for k in ("b1", "b2", "b3"))
    assert np.array_equal(np.round(d["W3"] * 16.0), d["W3"] * 16.0)
    exact = pr.forward(d, np.float64)
    got = br.forward_split(d, np.float64)
    assert np.array_equal(got["z1"], exact["z1"]) and np.array_equal(got["z2"], exact["z2"])
    # every operand splits exactly: head + tail is the value
    for v in (d["x"], d["W1"], d["W2"], exact["h1"].astype(np.float32)):
        h, t = split(v)
        assert np.array_equal(h.astype(np.float64) + t.astype(np.float64), v.astype(np.float64))
    assert np.array_equal(exact["h1"].astype(np.float32).astype(np.float64), exact["h1"])
    # exact in fp32 in ANY order: every partial sum is a multiple of 2^-11 (2^-17) below 2^13 (2^7)
    assert (np.abs(x) @ np.abs(W1).T + np.abs(b1)).max() < 2.0 ** 13
    assert (exact["h1"] @ np.abs(W2).T + np.abs(b2)).max() < 2.0 ** 7
    f32 = br.forward_split(d, np.float32, perm=True)
    assert np.array_equal(f32["z1"].astype(np.float64), exact["z1"]) and np.array_equal(f32["z2"].astype(np.float64), exact["z2"])
    # the masks are not a matter of rounding, and they are mixed
    for z in (exact["z1"], exact["z2"]):
        assert 0.1 < (z > 0).mean() < 0.9
    # the tails are exercised
    w1_tail = (split(d["W1"])[1] != 0).mean()
    h1_tail = (split(exact["h1"].astype(np.float32))[1] != 0).mean()
    z1_moved = (br.forward_split(d, np.float64, variant=("F1", "rt"))["z1"] != exact["z1"]).mean()
    z2_moved = (br.forward_split(d, np.float64, variant=("F2", "lt"))["z2"] != exact["z2"]).mean()
    print("F%d H%d/%d O%d: tails in %.2f of W1, %.2f of h1; no Wl.xh moves %.2f of z1, no Wh.xl %.2f of z2" % (net + (O, w1_tail, h1_tail, z1_moved, z2_moved)))
    assert 0.4 < w1_tail < 0.6 and h1_tail > 0.25 and z1_moved > 0.5 and z2_moved > 0.9


@HEADS
@pytest.mark.parametrize("case", br.SWEEP, ids=lambda c: "B%d-F%d-H%d-%d" % c)
def test_fp32_restatement_in_a_permuted_order_is_within_the_bound(case, O):
    r = br.reference(*case, O)
    got = br.evaluate(r["inputs"], np.float32, perm=True)
    for k in r["bound"]:
        w = pr.worst(got[k], r["ref"][k], r["bound"][k])
        assert w <= 1.0, (k, w)
    # and the bound is not vacuous: the split restatement in fp64 differs from the exact values somewhere in the gradient
    if case[0] >= 64:
        assert not np.array_equal(br.evaluate(r["inputs"], np.float64)["grad"], r["ref"]["grad"])


@HEADS
@pytest.mark.parametrize("variant", br.VARIANTS, ids=lambda v: "%s-%s" % v)
def test_every_wrong_variant_exceeds_the_bound(variant, O):
    r = br.reference(257, 51, 100, 100, O)
    got = br.evaluate(r["inputs"], np.float64, variant=variant)
    w = pr.worst(got["grad"], r["ref"]["grad"], r["bound"]["grad"])
    print("O%d without %s of %s: worst |error| / bound = %.1f" % (O, variant[1], variant[0], w))
    assert w > 1.0


@HEADS
@pytest.mark.parametrize("kind", ["x", "w2"])
@pytest.mark.parametrize("net", br.NETS, ids=lambda n: "F%d-H%d-%d" % n)
def test_the_further_grid_kinds_make_the_forward_exact_with_tails_in_x_or_in_w2(net, kind, O):
    """No product of the forward has a tail on both sides (the dropped al bl would make it inexact): "x" puts tails into x (and h1),
    "w2" into W2 with h1 exact in bf16."""
    d = br.draw(*net, O, kind=kind)
    x, W1, b1, W2, b2 = (d[k].astype(np.float64) for k in ("x", "W1", "b1", "W2", "b2"))
    exact = pr.forward(d, np.float64)
    h1 = exact["h1"].astype(np.float32)
    tail = lambda v: split(v)[1] != 0
    if kind == "x":
        assert np.array_equal(np.round(x * 512), x * 512) and np.abs(x).max() <= 1 and set(np.unique(W1)) <= {-0.25, 0.0, 0.25}
        assert np.array_equal(np.round(W2 * 64), W2 * 64) and np.abs(W2).max() <= 4 / 64
        assert not tail(d["W1"]).any() and not tail(d["W2"]).any() and tail(d["x"]).mean() > 0.15 and tail(h1).mean() > 0.15
        gran1, gran2 = 2.0 ** -11, 2.0 ** -17
    else:
        assert set(np.unique(x)) <= {-1.0, 0.0, 1.0} and np.array_equal(np.round(W1 * 16), W1 * 16) and np.abs(W1).max() <= 0.25
        assert np.array_equal(np.round(W2 * 8192), W2 * 8192) and np.abs(W2).max() <= 1 / 16
        assert not tail(d["x"]).any() and not tail(d["W1"]).any() and not tail(h1).any() and tail(d["W2"]).mean() > 0.15
        gran1, gran2 = 2.0 ** -5, 2.0 ** -18
    got = br.forward_split(d, np.float64)
    assert np.array_equal(got["z1"], exact["z1"]) and np.array_equal(got["z2"], exact["z2"])
    for v in (d["x"], d["W1"], d["W2"], h1):      # head + tail is the value
        h, t = split(v)
        assert np.array_equal(h.astype(np.float64) + t.astype(np.float64), v.astype(np.float64))
    assert np.array_equal(h1.astype(np.float64), exact["h1"])
    # exact in fp32 in ANY order: every partial sum is a multiple of the granularity, below 2^24 of it
    assert (np.abs(x) @ np.abs(W1).T + np.abs(b1)).max() < 2.0 ** 24 * gran1
    assert (exact["h1"] @ np.abs(W2).T + np.abs(b2)).max() < 2.0 ** 24 * gran2
    f32 = br.forward_split(d, np.float32, perm=True)
    assert np.array_equal(f32["z1"].astype(np.float64), exact["z1"]) and np.array_equal(f32["z2"].astype(np.float64), exact["z2"])
    for z in (exact["z1"], exact["z2"]):
        assert 0.1 < (z > 0).mean() < 0.9
    # the forward variant of the kind moves most of its z
    product, z = ("F1", "z1") if kind == "x" else ("F2", "z2")
    moved = (br.forward_split(d, np.float64, variant=(product, "lt" if kind == "x" else "rt"))[z] != exact[z]).mean()
    assert moved > 0.5, moved


@HEADS
@pytest.mark.parametrize("kind,case", br.SWEEP_KINDS, ids=lambda v: v if isinstance(v, str) else "B%d-F%d-H%d-%d" % v)
def test_fp32_restatement_is_within_the_bound_on_the_further_kinds(kind, case, O):
    r = br.reference(*case, O, kind)
    got = br.evaluate(r["inputs"], np.float32, perm=True)
    for k in r["bound"]:
        assert pr.worst(got[k], r["ref"][k], r["bound"][k]) <= 1.0, k


@HEADS
@pytest.mark.parametrize("kind,variant", [(k, v) for k in ("x", "w2") for v in br.GRID_VARIANTS[k]], ids=lambda v: v if isinstance(v, str) else "%s-%s" % v)
def test_every_wrong_variant_exceeds_the_bound_on_the_further_kinds(kind, variant, O):
    """With GRID_VARIANTS["w1"] above: every one of the ten cross terms is outside the bound on a case the GPU sweep runs."""
    r = br.reference(257, 51, 100, 100, O, kind)
    w = pr.worst(br.evaluate(r["inputs"], np.float64, variant=variant)["grad"], r["ref"]["grad"], r["bound"]["grad"])
    print("%s O%d without %s of %s: worst |error| / bound = %.1f" % (kind, O, variant[1], variant[0], w))
    assert w > 1.0
    # and a variant not listed for the kind changes nothing there
    for other in set(br.ALL_VARIANTS) - set(br.GRID_VARIANTS[kind]):
        assert np.array_equal(br.evaluate(r["inputs"], np.float64, variant=other)["grad"], br.evaluate(r["inputs"], np.float64)["grad"])


@HEADS
@pytest.mark.parametrize("net", FULL_NETS, ids=lambda n: "F%d-H%d-%d" % n)
def test_full_mantissa_inputs(net, O):
    """Seeded default-initialised networks, uniform states: at most a third of the rows risky (25 - 41 of 257 here), forward outputs
    and the kept rows' gradient within the bound.  The layer-2 Wl.xh variant and the layer-1 Wh.xl variant are outside the kept
    rows' GRADIENT bound, which the GPU test checks; the layer-2 one is also 4.9 - 5.8 x outside on z2.  On the forward outputs it
    is only 0.14 - 0.36 of the bound: that figure is printed, not asserted."""
    r = br.full_reference(*net, O)
    d, B = r["inputs"], br.PARENT_ROWS
    left_out = B - len(r["keep"])
    print("F%d H%d/%d O%d: %d of %d rows left out" % (net + (O, left_out, B)))
    assert 3 * left_out <= B
    # the split restatement in fp64 is within the forward bound of the exact values, the fp32 one in a permuted order too
    f32 = br.evaluate(d, np.float32, perm=True)
    for k in br.FORWARD_KEYS[O]:
        assert pr.worst(r["fwd_split"][k], r["fwd_exact"][k], r["fwd_bound"][k]) <= 1.0, k
        assert pr.worst(f32[k], r["fwd_exact"][k], r["fwd_bound"][k]) <= 1.0, k
    # The layer-2 Wl.xh variant is outside the bound where the bound is sharpest, on z2 itself.  At the outputs it is NOT: a dropped
    # cross term is about 2^-10 of each product with either sign, so it grows with the square root of the 100 x 100 terms between
    # h1 and a logit, while a worst-case bound (about 2^-15 of each product) grows with their number; the figure is printed.
    fw, _, E_z2, _ = br.forward_bound(d, False)
    bad = br.forward_split(d, np.float64, variant=br.VARIANT_L2_WL_XH)
    assert pr.worst(br.forward_split(d, np.float32, perm=True)["z2"], fw["z2"], E_z2) <= 1.0
    at_z2 = pr.worst(bad["z2"], fw["z2"], E_z2)
    out = "ratio" if O == 2 else "value"
    at_out = pr.worst(br.evaluate(d, np.float64, variant=br.VARIANT_L2_WL_XH)[out], r["fwd_exact"][out], r["fwd_bound"][out])
    print("F%d H%d/%d O%d: without Wl.xh of layer 2, worst |error| / bound = %.2f on z2, %.2f on the %s" % (net + (O, at_z2, at_out, out)))
    assert at_z2 > 1.0
    # on the kept rows the masks of the fp32 restatement are the exact ones and its gradient is within the bound
    kept = r["kept"]
    fw32, fw64 = br.forward_split(kept["inputs"], np.float32, perm=True), pr.forward(kept["inputs"], np.float64)
    assert np.array_equal(fw32["z1"] > 0, fw64["z1"] > 0) and np.array_equal(fw32["z2"] > 0, fw64["z2"] > 0)
    got = br.evaluate(kept["inputs"], np.float32, perm=True)
    for k in kept["bound"]:
        assert pr.worst(got[k], kept["ref"][k], kept["bound"][k]) <= 1.0, k
    # ... and that gradient check discriminates the two forward tails the "w1" grid cannot exercise: W2's in F2, x's in F1
    for variant in (br.VARIANT_L2_WL_XH, ("F1", "lt")):
        w = pr.worst(br.evaluate(kept["inputs"], np.float64, variant=variant)["grad"], kept["ref"]["grad"], kept["bound"]["grad"])
        print("F%d H%d/%d O%d: without %s of %s, kept rows' gradient: worst |error| / bound = %.1f" % (net + (O, variant[1], variant[0], w)))
        assert w > 1.0


def _declaration(text, name):
    args = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, text, flags=re.S).group(1)
    return [re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip() for a in args.split(",")]


@pytest.mark.parametrize("name", ["mdr_ppo_actor_grad", "mdr_ppo_critic_grad"])
def test_header_declares_and_native_binds_the_entry_points(name):
    text = _header()
    assert _declaration(text, name + "_bf16x3") == _declaration(text, name)
    assert len(_declaration(text, name)) == (15 if "actor" in name else 13)
    assert name + "_bf16x3" in nat.EXPORTS
    lib = nat.load()
    ours, theirs = getattr(lib, name + "_bf16x3"), getattr(lib, name)
    assert ours.argtypes == theirs.argtypes and ours.restype == theirs.restype
