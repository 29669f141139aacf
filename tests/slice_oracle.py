"""The fp64 oracle on a few slices of a device batch: OracleEnv(cfg, nb_envs=k, env_offset=off) for the first, middle and last
envs (or any given offsets), stepped with the device's own actions, and every step checked against the device with the contract of
tests/test_gpu_parity.py: integer state and cluster power exactly, temperatures to T_RTOL, rewards to R_RTOL + R_ATOL, the seven
observation planes to 2e-5 + 2e-6.  In-kernel controller decisions are checked against the oracle's rule on the oracle's state:
a house may decide otherwise only where the fp64 temperature lies within EDGE_RTOL of a threshold."""
import numpy as np
import torch

T_RTOL = 1e-5
R_RTOL, R_ATOL = 1e-5, 1e-5
OBS_RTOL, OBS_ATOL = 2e-5, 2e-6
EDGE_RTOL = 1e-5


def slice_offsets(E, k):
    """First, middle and last k envs of a batch of E (fewer slices where they would coincide)."""
    k = min(k, E)
    return sorted({0, (E - k) // 2, E - k}), k


class SliceOracle:
    def __init__(self, cfg, env, seed, episode, k=3, offsets=None, r_atol=R_ATOL):
        from oracle import mdr_oracle as mo
        E = env.nb_envs
        if offsets is None:
            offsets, k = slice_offsets(E, k)
        self.offsets, self.k = list(offsets), k
        assert all(0 <= o and o + k <= E for o in self.offsets)
        self.oras = [mo.OracleEnv(cfg, nb_envs=k, env_offset=o).reset(seed=seed, episode=episode) for o in self.offsets]
        self.idx = torch.tensor(np.concatenate([np.arange(o, o + k) for o in self.offsets]), dtype=torch.long, device=env.device)
        self.r_atol = r_atol
        self.rewards = [None] * len(self.oras)

    def take(self, t, dim=0):
        """The slices of a device tensor over envs (dim), as one numpy array per slice."""
        x = t.index_select(dim, self.idx).cpu().numpy()
        return np.split(x, len(self.offsets), axis=dim)

    def decisions(self, kind):
        """The oracle's controller decisions on its current state (bool per slice)."""
        return [getattr(o, kind + "_actions")() for o in self.oras]

    def near_threshold(self, kind):
        """Houses whose fp64 temperature lies within EDGE_RTOL of a threshold of the controller (bool per slice)."""
        out = []
        for o in self.oras:
            near = np.zeros(o.Ta.shape, dtype=bool)
            edges = () if kind == "always_on" else (o.target,) if kind == "bangbang" else (o.target - o.deadband / 2, o.target + o.deadband / 2)
            for edge in edges:
                near |= np.abs(o.Ta - edge) <= EDGE_RTOL * np.abs(edge)
            out.append(near)
        return out

    def decision_misses(self, device_actions, kind, ref=None):
        """(houses deciding otherwise, of those the ones NOT within EDGE_RTOL of a threshold) over all slices."""
        ref = self.decisions(kind) if ref is None else ref
        diff_n = off_edge_n = 0
        for dev, want, near in zip(device_actions, ref, self.near_threshold(kind)):
            diff = dev.astype(bool) != np.asarray(want, dtype=bool)
            diff_n += int(diff.sum())
            off_edge_n += int((diff & ~near).sum())
        return diff_n, off_edge_n

    def step(self, actions):
        self.rewards = [o.step(np.asarray(a).astype(np.uint8)) for o, a in zip(self.oras, actions)]

    def check(self, env, where="", reward=True, obs=True):
        """The contract on every slice; `where` goes into the failure message."""
        t = env.t
        flags = self.take(t["flags"])
        sso = self.take(t["sso"])
        P = self.take(t["P"])
        Ta, Tm = self.take(env.house_temp()), self.take(env.house_mass_temp())
        S, OD = self.take(env.reg_signal()), self.take(env.od_temp())
        rew = self.take(t["reward"]) if reward else None
        planes = self.take(t["obs"], dim=1) if obs and t["obs"].numel() else None
        for j, o in enumerate(self.oras):
            msg = "%s, envs [%d, %d)" % (where, self.offsets[j], self.offsets[j] + self.k)
            np.testing.assert_array_equal((flags[j] & 1).astype(bool), o.on, err_msg="on " + msg)
            np.testing.assert_array_equal((flags[j] & 2).astype(bool), o.lock, err_msg="lock " + msg)
            np.testing.assert_array_equal(sso[j], o.sso, err_msg="sso " + msg)
            np.testing.assert_array_equal(P[j], o.P, err_msg="P " + msg)
            np.testing.assert_allclose(Ta[j], o.Ta, rtol=T_RTOL, atol=0, err_msg="Ta " + msg)
            np.testing.assert_allclose(Tm[j], o.Tm, rtol=T_RTOL, atol=0, err_msg="Tm " + msg)
            np.testing.assert_allclose(S[j], o.S, rtol=1e-9, atol=1e-6, err_msg="signal " + msg)
            np.testing.assert_allclose(OD[j], o.OD, rtol=0, atol=5e-6, err_msg="outdoor temperature " + msg)
            if rew is not None and self.rewards[j] is not None:
                np.testing.assert_allclose(rew[j], self.rewards[j], rtol=R_RTOL, atol=self.r_atol, err_msg="reward " + msg)
            if planes is not None:
                np.testing.assert_allclose(planes[j], o.dynamic_obs(), rtol=OBS_RTOL, atol=OBS_ATOL, err_msg="obs planes " + msg)
