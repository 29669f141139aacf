"""FusedTarMACActor.sample (csrc/mdr_tarmac_mlp.hip, csrc/mdr_tarmac_mlp_bf16.hip) against its own recorded bits:
tests/golden/tarmac_mlp_parent_bits.npz holds ``action``, ``a_prob``, ``probs`` and the whole workspace (``cat``, ``qkv``, ``state``) of
one sample per case and precision, written by tests/golden/make_tarmac_mlp_bits.py on the MI355X at the commit before the encode
kernels, the head's tail and the launch chain were each folded into one.  There is no tolerance: same compiler, same flags
(-ffp-contract=on) and the same MFMA sequence give the same bits, and a mismatch means an operation order has changed - which the
fp64 probability contract of the other suites would let pass."""
import os

import numpy as np
import pytest

from tests.golden import make_tarmac_mlp_bits as gen

pytestmark = pytest.mark.gpu

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tarmac_mlp_parent_bits.npz"))


def test_the_fixture_holds_every_case():
    assert list(GOLDEN["names"]) == gen.case_names()
    assert len(str(GOLDEN["commit"])) == 40      # the commit the recorded bits were computed at


@pytest.mark.parametrize("name", gen.case_names())
def test_sample_bits_equal_the_recorded_ones(name):
    got = gen.run(name)
    for key in gen.ARRAYS:
        want = GOLDEN[name + "/" + key]
        assert got[key].dtype == want.dtype and got[key].shape == want.shape, key
        assert np.array_equal(got[key].view(np.uint8), want.view(np.uint8)), "%s: %s differs from the recorded bits" % (name, key)
    assert got["cat"].size and (got["qkv"].size > 0) == ("nocomm" not in name) and (got["state"].size > 0) == ("hops2" in name)
