#!/usr/bin/env python3
"""Runs the usage sketch of README.md (kept in sync by hand) - a quick end-to-end sanity run on a GPU box."""
import os
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mdr_amd  # noqa: E402

warnings.simplefilter("ignore")
cfg = mdr_amd.default_config()
cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = 20
env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=100_000, device="cuda:0", seed=1)
obs7 = env.reset()
state = env.obs_vector("rows")
actions = (torch.rand(env.nb_envs, env.nb_houses, device="cuda") < 0.5).to(torch.uint8)
obs7, reward, done, info = env.step(actions)
metrics = env.rollout_fused(1000, power_trace=True)
single = mdr_amd.MADemandResponseEnv(cfg)
o = single.reset()
o, r, d, i = single.step({k: True for k in o})
torch.cuda.synchronize()
print("ok", tuple(obs7.shape), tuple(state.shape), tuple(reward.shape), tuple(info["cluster_hvac_power"].shape),
      sorted(metrics), len(o), round(r[0], 4), float(env.t["base_power"][0]))

from mdr_amd.rollout import ActorMLP, collect_ppo_rollout, deploy_policy  # noqa: E402
from mdr_amd.policy import FusedActor  # noqa: E402
actor = ActorMLP(env.obs_vector_length()).cuda()
batch = collect_ppo_rollout(env, actor, nb_steps=8, store_states=False)
dm = deploy_policy(env, FusedActor.from_module(actor), nb_steps=10)
torch.cuda.synchronize()
print("policy ok", sorted(batch), tuple(batch["action"].shape), sorted(dm), float(dm["reward_sum"].mean()))

from mdr_amd.rollout import collect_tarmac_rollout  # noqa: E402
from mdr_amd.tarmac import TarMACActor, TarMACCritic  # noqa: E402
from mdr_amd.tarmac_ppo import TarMACPPOLearner  # noqa: E402
small = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=64, device="cuda:0", seed=1)
small.reset()
tarmac = TarMACActor(small.obs_vector_length()).cuda()
tarmac_critic = TarMACCritic(small.nb_houses, small.obs_vector_length()).cuda()
tbatch = collect_tarmac_rollout(small, tarmac, nb_steps=8, critic=tarmac_critic)
tarmac_learner = TarMACPPOLearner(tarmac, tarmac_critic, lr_actor=1e-3, lr_critic=1e-3, ppo_update_time=2)
a_loss, c_loss, n_mb = tarmac_learner.update(tbatch, seed=0)
torch.cuda.synchronize()
print("tarmac update ok", float(a_loss), float(c_loss), n_mb, tarmac_learner.uses_kernels(256))

from mdr_amd.dqn import DQNLearner, QNetworkMLP, train_dqn  # noqa: E402
dqn_learner = DQNLearner(QNetworkMLP(small.obs_vector_length()).cuda(), lr=1e-3, buffer_capacity=4096)
losses, epsilon = train_dqn(small, dqn_learner, nb_steps=4)
torch.cuda.synchronize()
print("dqn update ok", [round(float(x), 4) for x in losses], epsilon, len(dqn_learner.buffer), dqn_learner.uses_kernels(256))
