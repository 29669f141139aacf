#!/usr/bin/env python3
"""The per-step exchange of BASELINE config 5 (1 env x 1,000,000 houses) on ONE rank for the shares of 1, 2, 4, 8 ranks: us per
eager env.step(actions) through the records path (step_begin_records, RCCL all-gather of a world of one, step_end_records -
bench.py's c5 leg) and through sharding.MailboxExchange (one mdr_env_step_mailbox launch), their checksums after the same steps,
and us per step of collect_ppo_rollout (neighbours topology, fp32 fused actor, states kept) under each exchange.  One JSON line
per share."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
import bench
import mdr_amd
from mdr_amd import rollout as ro
from mdr_amd.sharding import MailboxExchange, TorchDistExchange

dev = torch.device("cuda", 0)
torch.cuda.set_device(dev)
K = int(os.environ.get("K", "400"))
KP = int(os.environ.get("KP", "8"))
shares = [int(s) for s in os.environ.get("SHARES", "1000000,500000,250000,125000").split(",")]
os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
os.environ.setdefault("MASTER_PORT", str(bench.free_port()))
sys.stdout.flush()
saved = os.dup(1)
os.dup2(2, 1)          # RCCL's banner goes to stderr: stdout keeps the JSON lines
dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
dist.barrier()
sys.stdout.flush()
os.dup2(saved, 1)


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


for share in shares:
    cfg = bench.c3_config(mdr_amd)
    cfg["default_env_prop"]["cluster_prop"]["nb_agents"] = share
    cfg["default_env_prop"]["cluster_prop"]["agents_comm_mode"] = "neighbours"
    row = {"houses_on_rank": share, "steps": K, "ppo_steps": KP, "backend": "rccl (world of one)"}
    gen = torch.Generator(device=dev).manual_seed(2024)
    acts = [(torch.rand((1, share), device=dev, generator=gen) < 0.5).to(torch.uint8) for _ in range(2)]
    for name, make in (("records", lambda: TorchDistExchange()), ("mailbox", lambda: MailboxExchange())):
        env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=1, device=dev, seed=2024, table_steps=64, house_shard=(0, share),
                                               exchange_always=True, exchange=make())
        env.reset(episode=0)

        def steps(n):
            for t in range(n):
                env.step(acts[t & 1])

        steps(20)
        row[name + "_step_us"] = round(timed(lambda: steps(K), K), 3)
        env.exchange_status()
        row["checksum_Ta_" + name] = float(env.t["Ta"].double().sum())
        torch.manual_seed(0)
        actor = ro.ActorMLP(env.obs_vector_length()).to(dev)
        ro.collect_ppo_rollout(env, actor, KP, seed=1)
        row[name + "_ppo_us_per_step"] = round(timed(lambda: ro.collect_ppo_rollout(env, actor, KP, seed=1), KP), 3)
        del env
        torch.cuda.empty_cache()
    row["checksums_equal"] = row["checksum_Ta_records"] == row["checksum_Ta_mailbox"]
    row["step_speedup"] = round(row["records_step_us"] / row["mailbox_step_us"], 3)
    print(json.dumps(row), flush=True)
dist.destroy_process_group()
