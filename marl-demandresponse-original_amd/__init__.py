"""MI355X-native batched demand-response environment step (import name: ``mdr_amd``).

Only what the hot path needs lives here: ``csrc/`` (HIP kernels + the C ABI of include/mdr.h), the ctypes
binding, the config schema and the host-side mirrors of the reference's env interface.
"""
from .config import default_config, flatten_config, EnvSpec  # noqa: F401
from ._native import LIB_PATH, NativeLibraryMissing, load as load_native  # noqa: F401
from .build import build_native  # noqa: F401


def __getattr__(name):
    # torch is imported lazily so that `import mdr_amd` (config, build) works in tools that only need the schema
    if name in ("BatchedDemandResponseEnv", "OBS_COLUMNS"):
        from . import batched_env
        return getattr(batched_env, name)
    if name in ("sharding", "comm", "rollout", "policy", "tarmac", "metrics", "montecarlo", "ppo", "tarmac_ppo", "dqn", "mappo", "maddpg", "mlp_actor", "optim", "tarmac_a2c", "graph_update"):      # submodules on first use (mdr_amd.sharding.house_shard ...)
        import importlib
        return importlib.import_module("." + name, __name__)
    if name == "BatchedMetrics":
        from .metrics import BatchedMetrics
        return BatchedMetrics
    if name in ("TarMACActor", "TarMACCritic", "FusedTarMACActor"):
        from . import tarmac
        return getattr(tarmac, name)
    if name == "PPOLearner":
        from .ppo import PPOLearner
        return PPOLearner
    if name == "MAPPOLearner":
        from .mappo import MAPPOLearner
        return MAPPOLearner
    if name in ("DQNLearner", "QNetworkMLP", "DeviceReplayBuffer"):
        from . import dqn
        return getattr(dqn, name)
    if name in ("MADDPGLearner", "DDPGNetworkMLP", "JointReplayBuffer", "GreedyDDPGActor", "train_maddpg"):
        from . import maddpg
        return getattr(maddpg, name)
    if name in ("FusedMLPActor", "FusedMLPActors"):
        from . import mlp_actor
        return getattr(mlp_actor, name)
    if name == "TarMACPPOLearner":
        from .tarmac_ppo import TarMACPPOLearner
        return TarMACPPOLearner
    if name in ("TarMACA2CPolicy", "TarMACA2CLearner"):
        from . import tarmac_a2c
        return getattr(tarmac_a2c, name)
    if name == "FusedAdam":
        from .optim import FusedAdam
        return FusedAdam
    if name == "MADemandResponseEnv":
        from .env import MADemandResponseEnv
        return MADemandResponseEnv
    raise AttributeError(name)
