"""mdr_env_bind_hvac_code without a GPU: the entry point is exported and refuses a NULL handle on the host, and the rule the
detection kernel implements - distinct raw-bit (Q_hvac, P_max) pairs, at most 16 - restated in numpy on the oracle's own sample."""
import numpy as np

import mdr_amd
from mdr_amd import _native as nat


def dictionary(Q_hvac, P_max, cap=nat.MDR_HVAC_DICT_ENTRIES):
    """The distinct (Q_hvac, P_max) pairs of fp32 arrays as 64-bit keys (P_max bits high), or None when there are more than `cap`
    or one of them is the all-ones key that marks a free slot."""
    q = np.ascontiguousarray(Q_hvac, dtype=np.float32).view(np.uint32).astype(np.uint64).ravel()
    p = np.ascontiguousarray(P_max, dtype=np.float32).view(np.uint32).astype(np.uint64).ravel()
    keys = np.unique((p << np.uint64(32)) | q)
    if len(keys) > cap or (keys == np.uint64(0xFFFFFFFFFFFFFFFF)).any():
        return None
    return keys


def test_entry_point_is_exported_and_host_checked():
    assert "mdr_env_bind_hvac_code" in nat.EXPORTS
    lib = mdr_amd.load_native()
    assert lib.mdr_env_bind_hvac_code(None, None, None) == nat.MDR_ERR_INVALID
    assert nat.MDR_HVAC_DICT_ENTRIES == nat.MDR_MAX_CAPACITIES == 16
    assert nat.MDR_HVAC_DICT_COUNT == 2 * nat.MDR_HVAC_DICT_ENTRIES < nat.MDR_HVAC_DICT_WORDS


def test_rule_is_bitwise_and_capped():
    q = np.array([1.0, 1.0, 1.0, 1.0], dtype=np.float32)
    p = np.array([0.0, -0.0, 2.0, 2.0], dtype=np.float32)
    assert len(dictionary(q, p)) == 3      # -0.0 is not +0.0; equal Q_hvac with different P_max are two entries
    many = np.arange(17, dtype=np.float32)
    assert len(dictionary(many[:16], many[:16])) == 16
    assert dictionary(many, many) is None
    free = np.array([0xFFFFFFFF], dtype=np.uint32).view(np.float32)
    assert dictionary(free, free) is None


def test_c3_sample_of_the_oracle_has_five_pairs():
    """The benchmark's configuration as the oracle samples it (utils.apply_hvac_noise draws the capacity from a list of five and
    leaves COP and the latent fraction alone): five pairs over the batch."""
    import bench
    from oracle import mdr_oracle as mo
    ora = mo.OracleEnv(bench.c3_config(mdr_amd), nb_envs=4).reset(seed=2024, episode=0)
    keys = dictionary(ora.Qhvac, ora.Pmax)
    assert keys is not None and len(keys) == 5
    assert sorted(np.unique(ora.capacity).tolist()) == [10000.0, 12500.0, 15000.0, 17500.0, 20000.0]
    assert len(np.unique(ora.COP)) == 1 and len(np.unique(ora.latent)) == 1
