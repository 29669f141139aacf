"""Sharded houses through sharding.MailboxExchange: one launch per externally driven step (mdr_env_step_mailbox,
csrc/mdr_mailbox.hip) and the neighbour-message halo through the same mailboxes, held bit for bit to the records path
(step_begin_records / all-gather / step_end_records) it replaces, and the policy loops of train_ppo.py:62-77,
train_dqn.py:55-91 and main-deploy.py:99-152 on a sharded env.  env/MA_DemandResponse.py:1042-1050 (cluster power),
274-321 (common penalties), 976-1001 (messages)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STATE = ("Ta", "Tm", "sso", "flags", "actions", "reward", "obs", "P")


def _cfg(n, mode="individual_L2", signal="sinusoidals", topology="neighbours", defect=0.0, hvac_messages=False):
    import mdr_amd
    cfg = mdr_amd.default_config()
    env = cfg["default_env_prop"]
    env["cluster_prop"]["nb_agents"] = n
    env["cluster_prop"]["agents_comm_mode"] = topology
    env["cluster_prop"]["comm_defect_prob"] = defect
    env["message_properties"]["hvac"] = hvac_messages
    env["power_grid_prop"]["base_power_mode"] = "constant"
    env["power_grid_prop"]["signal_mode"] = signal
    env["reward_prop"]["temp_penalty_mode"] = mode
    cfg["noise_house_prop"]["noise_mode"] = "big_noise"
    cfg["noise_hvac_prop"]["noise_mode"] = "big_noise"
    return cfg


class _OneShard:
    """Exchange of a world of one without torch.distributed: the records path on the shard's own `partials`."""

    def agree_partial_records(self, env):
        pass

    def sum_max_power(self, env):
        pass

    def sum_base_power(self, env):
        pass

    def gather_partials(self, env):
        return env.t["partials"].unsqueeze(0), 1

    def ranges(self, env):
        return [(0, env.nb_agents)], 0

    def gather_messages(self, env, padded):
        return padded.unsqueeze(0).clone()


def _pair(cfg, E, N, seed, **kw):
    """(records path, mailbox path) envs of a world of one over the same N houses."""
    import mdr_amd
    from mdr_amd.sharding import MailboxExchange
    rec = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=16, house_shard=(0, N),
                                           exchange_always=True, exchange=_OneShard(), **kw)
    mbx = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=16, house_shard=(0, N),
                                           exchange_always=True, exchange=MailboxExchange(), **kw)
    return rec, mbx


def _same(a, b, where):
    for name in STATE:
        assert torch.equal(a.t[name], b.t[name]), (where, name)
    assert torch.equal(a.reg_signal(), b.reg_signal()), where


# ---------------------------------------------------------------------------------------------------------------- section 0
@pytest.mark.parametrize("exchange", ["records", "mailbox"])
def test_policy_loops_run_on_a_sharded_env(exchange, monkeypatch):
    """collect_ppo_rollout (states kept), collect_dqn_transitions and deploy_policy on a world-of-one shard - they observe into
    caller buffers - against the same calls on the unsharded env through the same (rows-form) policy kernel."""
    import mdr_amd
    from mdr_amd import rollout as ro
    from mdr_amd.policy import FusedActor
    from mdr_amd.sharding import MailboxExchange
    E, N, T = 2, 6000, 16
    cfg = _cfg(N, "common_L2")
    ex = _OneShard() if exchange == "records" else MailboxExchange()
    shd = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=11, table_steps=16, house_shard=(0, N),
                                           exchange_always=True, exchange=ex)
    ref = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=11, table_steps=16)
    F = ref.obs_vector_length()
    torch.manual_seed(0)
    actor = ro.ActorMLP(F).to("cuda:0")
    qnet = ro.ActorMLP(F).to("cuda:0")
    monkeypatch.setattr(ro, "_observe_act_supported", lambda env, net: False)      # the rows form on both sides

    def same_state():
        for name in ("Ta", "Tm", "sso", "flags", "P"):
            assert torch.equal(shd.t[name], ref.t[name]), name

    ref.reset(episode=1)
    shd.reset(episode=1)
    a = ro.collect_ppo_rollout(ref, actor, T, seed=5, observe_act=False)
    b = ro.collect_ppo_rollout(shd, actor, T, seed=5)
    for key in ("state", "action", "a_prob", "done"):
        assert torch.equal(a[key], b[key]), key
    torch.testing.assert_close(b["reward"], a["reward"], rtol=1e-5, atol=1e-6)
    same_state()
    a = ro.collect_dqn_transitions(ref, qnet, T, epsilon=0.3, seed=4)
    b = ro.collect_dqn_transitions(shd, qnet, T, epsilon=0.3, seed=4)
    for key in ("state", "action", "explored"):
        assert torch.equal(a[key], b[key]), key
    torch.testing.assert_close(b["reward"], a["reward"], rtol=1e-5, atol=1e-6)
    same_state()
    pol = FusedActor.from_module(actor, device="cuda:0")
    a = ro.deploy_policy(ref, pol, T, seed=3)
    b = ro.deploy_policy(shd, pol, T, seed=3)
    same_state()
    torch.testing.assert_close(b["reward_sum"], a["reward_sum"], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(b["sq_signal_error_sum"], a["sq_signal_error_sum"], rtol=1e-12, atol=0)
    torch.testing.assert_close(b["sq_temp_error_sum"], a["sq_temp_error_sum"], rtol=1e-12, atol=0)
    with pytest.raises(ValueError, match="sharded"):
        ro.deploy_policy(shd, pol, 2, use_graph=True)


# ---------------------------------------------------------------------------------------------------------------- world of one
@pytest.mark.parametrize("E,N,mode,kind", [
    (1, 20000, "individual_L2", "external"),     # 20 house workgroups + the reducer; three table windows of 16 steps
    (3, 5000, "mixture", "bangbang"),            # several envs, every record field travels; every third step in-kernel bang-bang
    (2, 4099, "common_L2", "external"),          # nb_houses % 4 != 0: one house per lane, 256-house records
    (4, 300, "common_max", "no_planes"),         # one house workgroup per env; obs_planes=False
    (1, 300000, "mixture", "external"),          # 293 records: more than one per reducer thread
])
def test_mailbox_step_equals_records_path(E, N, mode, kind):
    T = 41
    rec, mbx = _pair(_cfg(N, mode), E, N, 23, obs_planes=kind != "no_planes")
    rec.reset(episode=2)
    mbx.reset(episode=2)
    gen = torch.Generator(device="cuda:0").manual_seed(N)
    for t in range(T):
        if kind == "bangbang" and t % 3 == 2:
            rec.step_bangbang()
            mbx.step_bangbang()
        else:
            act = (torch.rand((E, N), device="cuda:0", generator=gen) < 0.55).to(torch.uint8)
            rec.step(act)
            mbx.step(act)
        _same(rec, mbx, "step %d" % t)
    assert mbx.steps_taken == T
    assert mbx.exchange_status() == 0


def test_mailbox_step_vs_oracle():
    """The new kernel form on its own against the fp64 oracle (the contract of test_gpu_parity.py), 70 steps over four table windows."""
    import mdr_amd
    from mdr_amd.sharding import MailboxExchange
    from tests.slice_oracle import SliceOracle
    E, N, T, seed, episode = 4, 1500, 70, 4242, 1
    cfg = _cfg(N, "mixture")
    env = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=16, house_shard=(0, N),
                                           exchange_always=True, exchange=MailboxExchange())
    env.reset(episode=episode)
    sl = SliceOracle(cfg, env, seed, episode)
    sl.check(env, "after reset", reward=False, obs=False)
    gen = torch.Generator(device="cuda:0").manual_seed(7)
    for t in range(T):
        act = (torch.rand((E, N), device="cuda:0", generator=gen) < 0.55).to(torch.uint8)
        env.step(act)
        sl.step(sl.take(act))
        sl.check(env, "mailbox step %d" % t)
    assert env.exchange_status() == 0


def test_mailbox_steps_mix_with_the_persistent_rollout_world_of_one():
    rec, mbx = _pair(_cfg(20000, "common_max"), 1, 20000, 5)
    rec.reset(episode=0)
    mbx.reset(episode=0)
    _mix(rec, mbx, torch.Generator(device="cuda:0").manual_seed(1))
    assert mbx.exchange_status() == 0


def _mix(rec, mbx, gen, full=None, shard=None):
    E, N = mbx.nb_envs, mbx.nb_houses

    def act():
        a = (torch.rand((E, full or N), device="cuda:0", generator=gen) < 0.5).to(torch.uint8)
        return a if shard is None else a[:, shard[0]:shard[0] + shard[1]].contiguous()

    for t in range(10):
        a = act()
        rec.step(a)
        mbx.step(a)
    rec.rollout_persistent(20, accumulate=False)
    mbx.rollout_persistent(20, accumulate=False)
    _same(rec, mbx, "after the persistent rollout")
    for t in range(10):
        a = act()
        rec.step(a)
        mbx.step(a)
        _same(rec, mbx, "step %d after the persistent rollout" % t)


# ---------------------------------------------------------------------------------------------------------------- error paths
def test_a_missing_peer_ends_in_an_error_word_not_a_hang():
    """World of two whose peer mailbox is a zero-filled ghost nobody serves: the bounded wait gives up after a few ms, the error
    word (kind 3 / 4: the step path) lands in both mailboxes, the env keeps its state, and later launches write nothing."""
    import mdr_amd
    from mdr_amd import _native as nat
    from mdr_amd.sharding import MailboxExchange, Mailboxes
    N = 12000
    env = mdr_amd.BatchedDemandResponseEnv(_cfg(N), nb_envs=1, device="cuda:0", seed=3, house_shard=(0, N), exchange_always=True,
                                           exchange=MailboxExchange(timeout_ms=5))
    env.reset(episode=0)
    one = env._mailboxes
    ghost = torch.zeros_like(one.mem)
    two = nat.MdrMailbox()
    C.memmove(C.byref(two), C.byref(one.mb), C.sizeof(nat.MdrMailbox))
    two.world = 2
    two.records[1] = one.mb.records[0]
    two.boxes[1] = ghost.data_ptr()
    env._mailboxes = Mailboxes(env, two, [one.own, ghost.data_ptr()], one.mem)
    before = {k: env.t[k].clone() for k in ("Ta", "Tm", "sso", "flags", "reward")}
    act = torch.ones((1, N), dtype=torch.uint8, device="cuda:0")
    env.step(act)                                     # returns; the wait inside is bounded
    word = env.persist_status()
    assert word != 0
    assert (word >> 28) & 0xF in (3, 4)
    assert int(ghost[0].item()) != 0                  # the peer is told as well
    for k, v in before.items():
        assert torch.equal(env.t[k], v), k
    with pytest.raises(RuntimeError, match="rebuild"):
        env.exchange_status()
    env.step(act)                                     # finds the word set: leaves without writing
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(env.t[k], v), k


def test_a_grid_that_cannot_be_resident_is_refused():
    import mdr_amd
    from mdr_amd.sharding import MailboxExchange
    E, N = 600, 5000                                   # 600 x (5 + 1) workgroups
    env = mdr_amd.BatchedDemandResponseEnv(_cfg(N), nb_envs=E, device="cuda:0", seed=3, house_shard=(0, N), exchange_always=True,
                                           exchange=MailboxExchange())
    ref = mdr_amd.BatchedDemandResponseEnv(_cfg(N), nb_envs=E, device="cuda:0", seed=3, house_shard=(0, N), exchange_always=True,
                                           exchange=_OneShard())
    env.reset(episode=0)
    ref.reset(episode=0)
    act = torch.ones((E, N), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="exceed"):
        env.step(act)
    assert env.steps_taken == 0
    env._exchange_impl = _OneShard()                   # the handle is untouched: the records path steps on
    env.step(act)
    ref.step(act)
    _same(ref, env, "records step after the refusal")


# ---------------------------------------------------------------------------------------------------------------- ranks over hipIpc
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _init(rank, world, port):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      MDR_MAILBOX_CO_RESIDENT=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    return dist


def _ranks_pair(cfg, E, N, world, rank, seed):
    import mdr_amd
    from mdr_amd.sharding import MailboxExchange, house_shard
    shard = house_shard(N, world, rank)
    one = world == 1      # a world of one runs the exchanges all the same
    rec = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=16, house_shard=shard,
                                           exchange_always=one)
    mbx = mdr_amd.BatchedDemandResponseEnv(cfg, nb_envs=E, device="cuda:0", seed=seed, table_steps=16, house_shard=shard,
                                           exchange_always=one, exchange=MailboxExchange())
    return rec, mbx, shard


def _ipc_worker(rank, world, port, N, mode, E, topology, defect, hvac_messages):
    dist = _init(rank, world, port)
    rec, mbx, shard = _ranks_pair(_cfg(N, mode, topology=topology, defect=defect, hvac_messages=hvac_messages), E, N, world, rank, 17)
    rec.reset(episode=1)
    mbx.reset(episode=1)
    gen = torch.Generator(device="cuda:0").manual_seed(99)
    for t in range(40):
        act = (torch.rand((E, N), device="cuda:0", generator=gen) < 0.5).to(torch.uint8)[:, shard[0]:shard[0] + shard[1]].contiguous()
        rec.step(act)
        mbx.step(act)
        _same(rec, mbx, (rank, t))
        if t % 13 == 0:
            assert torch.equal(rec.obs_vector("rows"), mbx.obs_vector("rows")), (rank, t)
    assert torch.equal(rec.obs_vector("rows"), mbx.obs_vector("rows")), rank
    assert mbx.exchange_status() == 0
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("N,world,mode,E,topology,defect,hvac", [
    (20000, 2, "individual_L2", 1, "neighbours", 0.0, False),
    (30000, 3, "mixture", 2, "closed_groups", 0.0, False),
    (9001, 4, "common_L2", 1, "neighbours", 0.2, False),          # link defects, drawn per global house index
    (500000, 4, "individual_L2", 1, "neighbours", 0.0, True),     # message columns: F = 81
])
def test_ranks_on_one_gpu_step_and_observe_through_ipc_mailboxes(N, world, mode, E, topology, defect, hvac):
    """2-4 ranks (one process each) on the one GPU, mailboxes mapped into each other over hipIpc: every step's state, signal and
    rewards, and the observation rows with their halo, bit-identical to the records path over a gloo all-gather."""
    import torch.multiprocessing as mp
    mp.spawn(_ipc_worker, args=(world, _free_port(), N, mode, E, topology, defect, hvac), nprocs=world, join=True)


def _no_collective_worker(rank, world, port):
    import torch.distributed as dist_mod
    from mdr_amd import rollout as ro
    from mdr_amd.policy import FusedActor
    dist = _init(rank, world, port)
    N, E, T = 8000, 1, 16
    rec, mbx, shard = _ranks_pair(_cfg(N, "common_L2"), E, N, world, rank, 29)
    F = rec.obs_vector_length()
    torch.manual_seed(0)
    actor = ro.ActorMLP(F).to("cuda:0")
    pol = FusedActor.from_module(actor, device="cuda:0")
    names = ("all_gather_into_tensor", "all_gather", "all_reduce", "broadcast")
    for run in ("ppo", "deploy"):
        rec.reset(episode=3)
        mbx.reset(episode=3)
        counts = dict.fromkeys(names, 0)
        saved = {n: getattr(dist_mod, n) for n in names}

        def counting(n):
            def f(*a, **k):
                counts[n] += 1
                return saved[n](*a, **k)
            return f

        for n in names:
            setattr(dist_mod, n, counting(n))
        try:
            got = ro.collect_ppo_rollout(mbx, actor, T, seed=1) if run == "ppo" else ro.deploy_policy(mbx, pol, T, seed=1)
        finally:
            for n in names:
                setattr(dist_mod, n, saved[n])
        assert all(v == 0 for v in counts.values()), (rank, run, counts)
        want = ro.collect_ppo_rollout(rec, actor, T, seed=1) if run == "ppo" else ro.deploy_policy(rec, pol, T, seed=1)
        for key in want:
            assert torch.equal(got[key], want[key]), (rank, run, key)
        _same(rec, mbx, (rank, run))
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2])
def test_policy_loops_through_the_mailbox_run_no_collective(world):
    import torch.multiprocessing as mp
    mp.spawn(_no_collective_worker, args=(world, _free_port()), nprocs=world, join=True)


def _mix_worker(rank, world, port):
    dist = _init(rank, world, port)
    N = 30000
    rec, mbx, shard = _ranks_pair(_cfg(N, "mixture"), 1, N, world, rank, 41)
    rec.reset(episode=0)
    mbx.reset(episode=0)
    _mix(rec, mbx, torch.Generator(device="cuda:0").manual_seed(2), full=N, shard=shard)
    assert mbx.exchange_status() == 0
    torch.cuda.synchronize()
    dist.barrier()
    dist.destroy_process_group()


def test_mailbox_steps_mix_with_the_persistent_rollout_world_of_two():
    import torch.multiprocessing as mp
    mp.spawn(_mix_worker, args=(2, _free_port()), nprocs=2, join=True)
