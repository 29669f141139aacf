"""ctypes binding of libmdr_hip.so (include/mdr.h).  Loading fails loudly: there is no CPU fallback.

The structures below mirror ``mdr_config_t`` / ``mdr_buffers_t`` / ``mdr_episode_t`` field for field;
tests/test_abi.py parses include/mdr.h and checks names and order, and the library itself checks the
sizes (``struct_size``).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import gc
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MDR_HIP_LIB") or os.path.join(HERE, "csrc", "libmdr_hip.so")   # MDR_HIP_LIB: experiment builds


@contextlib.contextmanager
def gc_paused():
    """No cyclic garbage collection inside the block: what a stream capture runs under.  A collection that starts between two
    launches of a capture destroys whatever dead cycles earlier work left behind - a learner and its update graph hold each other,
    an env holds its library handle - and their destructors free device memory and destroy streams and graphs, runtime calls a
    capture in progress does not allow: the process aborts.  The garbage is collected as usual once the block is left."""
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


MDR_ABI_VERSION = 5
MDR_MAX_SINUSOIDS = 8
MDR_MAX_CAPACITIES = 16
MDR_HVAC_DICT_ENTRIES, MDR_HVAC_DICT_COUNT, MDR_HVAC_DICT_WORDS = 16, 32, 36   # mdr_env_bind_hvac_code
MDR_THERMAL_BITS = (25, 25, 25, 28, 25)   # mdr_env_bind_thermal_pack: field widths of k01, s0, k10, s1, inv_Ua in the 128-bit record
MDR_THERMAL_DESC_PACKED, MDR_THERMAL_DESC_BASE, MDR_THERMAL_DESC_WORDS = 0, 1, 32
MDR_OBS_COLUMNS = 7
MDR_MAX_SHARDS = 8

MDR_OK, MDR_ERR_INVALID, MDR_ERR_UNBOUND, MDR_ERR_HIP, MDR_ERR_UNSUPPORTED = 0, -1, -2, -3, -4
ACTIONS_EXTERNAL, ACTIONS_BANGBANG, ACTIONS_DEADBAND, ACTIONS_ALWAYS_ON = 0, 1, 2, 3
CONTROLLERS = {"bangbang": ACTIONS_BANGBANG, "deadband": ACTIONS_DEADBAND, "basic": ACTIONS_DEADBAND, "always_on": ACTIONS_ALWAYS_ON}

_f32p, _i32p, _u8p, _f64p, _i64p = (C.c_void_p,) * 5  # device pointers travel as plain addresses


class MdrConfig(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("nb_envs", C.c_int32), ("nb_houses", C.c_int32),
        ("nb_houses_total", C.c_int64), ("env_offset", C.c_int64), ("house_offset", C.c_int64),
        ("time_step", C.c_int32), ("table_steps", C.c_int32), ("temp_ref", C.c_double),
        ("init_air_temp", C.c_double), ("init_mass_temp", C.c_double), ("target_temp", C.c_double),
        ("deadband", C.c_double),
        ("Ua", C.c_double), ("Cm", C.c_double), ("Ca", C.c_double), ("Hm", C.c_double),
        ("window_area", C.c_double), ("shading_coeff", C.c_double), ("solar_gain", C.c_int32),
        ("lockout_duration", C.c_int32), ("lockout_noise", C.c_int32),
        ("COP", C.c_double), ("cooling_capacity", C.c_double), ("latent_cooling_fraction", C.c_double),
        ("std_start_temp", C.c_double), ("std_target_temp", C.c_double),
        ("factor_thermo_low", C.c_double), ("factor_thermo_high", C.c_double),
        ("nb_capacities", C.c_int32), ("start_random", C.c_int32),
        ("capacity_list", C.c_double * MDR_MAX_CAPACITIES),
        ("start_epoch", C.c_int64),
        ("day_temp", C.c_double), ("night_temp", C.c_double), ("temp_std", C.c_double),
        ("random_phase_offset", C.c_int32), ("signal_mode", C.c_int32),
        ("avg_power_per_hvac", C.c_double),
        ("nb_sinusoids", C.c_int32), ("perlin_nb_octaves", C.c_int32),
        ("sin_periods", C.c_double * MDR_MAX_SINUSOIDS), ("sin_amplitude_ratios", C.c_double * MDR_MAX_SINUSOIDS),
        ("steps_amplitude_per_hvac", C.c_double), ("steps_period", C.c_double),
        ("perlin_amplitude", C.c_double), ("perlin_octaves_step", C.c_double), ("perlin_period", C.c_double),
        ("artificial_ratio", C.c_double), ("artificial_signal_ratio_range", C.c_double),
        ("alpha_temp", C.c_double), ("alpha_sig", C.c_double),
        ("norm_temp_penalty", C.c_double), ("norm_sig_penalty", C.c_double),
        ("penalty_mode", C.c_int32), ("base_power_mode", C.c_int32),
        ("mix_ind_L2", C.c_double), ("mix_common_L2", C.c_double), ("mix_common_max", C.c_double),
        ("obs_power_norm", C.c_double),
    ]


class MdrBuffers(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
        ("Ta", _f32p), ("Tm", _f32p), ("sso", _i32p), ("flags", _u8p),
        ("k01", _f32p), ("s0", _f32p), ("k10", _f32p), ("s1", _f32p),
        ("inv_Ua", _f32p), ("Q_hvac", _f32p), ("P_max", _f32p),
        ("target", _f32p), ("deadband", _f32p), ("lockout", _i32p),
        ("Ua", _f32p), ("Cm", _f32p), ("Ca", _f32p), ("Hm", _f32p),
        ("capacity", _f32p), ("COP", _f32p), ("latent", _f32p),
        ("reward", _f32p), ("obs", _f32p),
        ("t0", _i64p), ("phase", _f64p), ("ratio", _f64p), ("max_power", _f64p),
        ("P", _f64p), ("tot_sum", _f64p), ("tot_max", _f64p),
        ("tab_od", _f32p), ("tab_solar", _f32p), ("tab_signal", _f64p),
        ("partials", _f64p), ("base_power", _f64p), ("cursor", C.c_void_p), ("tab_abs_noise", _f64p),
        ("pen_stash", _f32p),
        ("tab2_od", _f32p), ("tab2_solar", _f32p), ("tab2_signal", _f64p), ("tab2_abs_noise", _f64p),
        ("param_uniform", C.c_void_p),
    ]


class MdrEpisode(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
        ("Ta", _f64p), ("Tm", _f64p), ("target", _f64p), ("deadband", _f64p),
        ("Ua", _f64p), ("Cm", _f64p), ("Ca", _f64p), ("Hm", _f64p),
        ("capacity", _f64p), ("COP", _f64p), ("latent", _f64p),
        ("lockout", _i64p), ("t0", _i64p), ("phase", _f64p), ("ratio", _f64p),
    ]


class MdrObsSpec(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("layout", C.c_int32),
        ("state_hour", C.c_int32), ("state_day", C.c_int32), ("state_solar_gain", C.c_int32),
        ("state_thermal", C.c_int32), ("state_hvac", C.c_int32),
        ("message_thermal", C.c_int32), ("message_hvac", C.c_int32),
        ("nb_comm", C.c_int32),
        ("links", _i32p),
        ("random_links", C.c_int32), ("reserved0", C.c_int32),
        ("comm_defect_prob", C.c_double),
        ("out_plane_stride", C.c_int64),
        ("def_Ua", C.c_double), ("def_Cm", C.c_double), ("def_Ca", C.c_double), ("def_Hm", C.c_double),
        ("def_COP", C.c_double), ("def_capacity", C.c_double), ("def_latent", C.c_double), ("norm_reg_sig", C.c_double),
    ]


MDR_INTERP_AXES, MDR_INTERP_MAX_AXIS = 10, 16


class MdrInterpGrid(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("update_period", C.c_int32), ("nb_agents", C.c_int32), ("reserved0", C.c_int32),
        ("values", _f64p),
        ("dims", C.c_int32 * MDR_INTERP_AXES),
        ("axes", (C.c_double * MDR_INTERP_MAX_AXIS) * MDR_INTERP_AXES),
    ]


class MdrRolloutOut(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("reserved0", C.c_uint32),
        ("power_trace", _f64p), ("reward_sum", _f32p), ("sq_temp_error_sum", _f64p), ("sq_signal_error_sum", _f64p),
    ]


class MdrMailbox(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("world", C.c_int32), ("rank", C.c_int32), ("records_per_env", C.c_int32),
        ("records", C.c_int32 * MDR_MAX_SHARDS),
        ("system_scope", C.c_int32), ("co_resident", C.c_int32), ("spin_limit", C.c_uint32), ("reserved0", C.c_uint32),
        ("boxes", C.c_void_p * MDR_MAX_SHARDS),
    ]


class MdrMlp(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_state", C.c_int32), ("hidden1", C.c_int32), ("hidden2", C.c_int32), ("num_out", C.c_int32),
        ("w1", _f32p), ("b1", _f32p), ("w2", _f32p), ("b2", _f32p), ("w3", _f32p), ("b3", _f32p),
    ]


class MdrTarmacNet(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_state", C.c_int32), ("hidden", C.c_int32), ("num_key", C.c_int32), ("num_value", C.c_int32),
        ("nb_comm", C.c_int32), ("mode", C.c_int32), ("num_hops", C.c_int32), ("with_comm", C.c_int32), ("defect_prob", C.c_float),
        ("encode_w0", _f32p), ("encode_b0", _f32p), ("encode_w2", _f32p), ("encode_b2", _f32p),
        ("head_w0", _f32p), ("head_b0", _f32p), ("head_w2", _f32p), ("head_b2", _f32p),
        ("key_w0", _f32p), ("key_b0", _f32p), ("key_w2", _f32p), ("key_b2", _f32p),
        ("value_w0", _f32p), ("value_b0", _f32p), ("value_w2", _f32p), ("value_b2", _f32p),
        ("query_w0", _f32p), ("query_b0", _f32p), ("query_w2", _f32p), ("query_b2", _f32p),
    ]


class MdrTarmacA2CNet(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32), ("num_obs", C.c_int32), ("num_comm", C.c_int32), ("state_size", C.c_int32), ("num_key", C.c_int32),
        ("common_w0", _f32p), ("common_b0", _f32p), ("common_w2", _f32p), ("common_b2", _f32p),
        ("critic_w0", _f32p), ("critic_b0", _f32p), ("critic_w3", _f32p), ("critic_b3", _f32p),
        ("query_w", _f32p), ("query_b", _f32p), ("key_w", _f32p), ("key_b", _f32p), ("value_w", _f32p), ("value_b", _f32p),
        ("dist_w", _f32p),
    ]


MDR_ADAM_MAX_SEGMENTS = 32
MDR_MAX_AGENT_NETS = 32      # include/mdr_policy.h: nets per call of mdr_mlp_actors_sample / mdr_maddpg_target_agents / mdr_maddpg_*_all
MDR_MADDPG_DRAWS_MAX_AGENTS = 426      # include/mdr_policy.h: agents per call of mdr_maddpg_draws


class MdrAdamSegment(C.Structure):
    _fields_ = [("param", _f32p), ("grad", _f32p), ("target", _f32p), ("count", C.c_int64)]


class MdrAdamSegments(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("nb_segments", C.c_int32), ("seg", MdrAdamSegment * MDR_ADAM_MAX_SEGMENTS)]


OBS_PLANES, OBS_ROWS = 0, 1

EXPORTS = (
    "mdr_abi_version", "mdr_status_string", "mdr_last_error", "mdr_partials_per_env", "mdr_env_partial_records",
    "mdr_env_create", "mdr_env_destroy", "mdr_env_bind", "mdr_env_reset", "mdr_env_load_episode", "mdr_env_params_changed", "mdr_env_bind_hvac_code",
    "mdr_env_bind_thermal_pack", "mdr_env_rollout_plan", "mdr_env_rollout_resident",
    "mdr_rollout_rows", "mdr_env_bind_rollout_rows", "mdr_env_rollout_steps_per_launch", "mdr_env_fill_rollout_rows",
    "mdr_env_set_od_table", "mdr_env_set_interp_grid", "mdr_env_begin_episode", "mdr_env_refresh_obs", "mdr_env_step", "mdr_env_rollout", "mdr_env_rollout_fused",
    "mdr_env_step_begin", "mdr_env_step_end", "mdr_env_step_end_gathered", "mdr_env_step_begin_records", "mdr_env_step_end_records", "mdr_env_step_end_begin_records",
    "mdr_env_interp_due", "mdr_env_interp_local", "mdr_env_interp_apply", "mdr_obs_vector_length", "mdr_env_obs_vector",
    "mdr_obs_message_fields", "mdr_env_obs_messages", "mdr_env_obs_vector_ext", "mdr_env_comm_draws",
    "mdr_env_graph_room", "mdr_env_graph_replayed", "mdr_env_pack", "mdr_env_cursor", "mdr_env_set_cursor", "mdr_env_active_tables",
    "mdr_env_set_controller", "mdr_env_greedy_myopic_actions", "mdr_mailbox_bytes", "mdr_persist_records", "mdr_env_rollout_persistent",
    "mdr_mailbox_alloc", "mdr_mailbox_free", "mdr_mailbox_export", "mdr_mailbox_open", "mdr_mailbox_close", "mdr_mailbox_peek",
    "mdr_env_step_mailbox", "mdr_mailbox_halo_bytes", "mdr_mailbox_halo_push", "mdr_mailbox_halo_pull",
    # include/mdr_policy.h
    "mdr_actor_steps1", "mdr_actor_steps1_order", "mdr_actor_steps2", "mdr_actor_frag1_floats", "mdr_actor_frag2_floats", "mdr_actor_sample", "mdr_env_actor_sample", "mdr_env_actor_sample_links",
    "mdr_discounted_returns", "mdr_tarmac_comm", "mdr_logits_sample", "mdr_tarmac_comm_backward", "mdr_tarmac_comm_backward_workspace_bytes",
    "mdr_tarmac_comm_keyed", "mdr_tarmac_comm_backward_keyed",
    "mdr_tarmac_gather", "mdr_tarmac_gather_backward", "mdr_tarmac_gather_backward_workspace_bytes",
    "mdr_tarmac_frag_encode_floats", "mdr_tarmac_frag_proj_floats", "mdr_tarmac_frag_msg_floats", "mdr_tarmac_frag_head_floats",
    "mdr_tarmac_vec_floats", "mdr_tarmac_frag_words", "mdr_tarmac_actor_workspace_bytes", "mdr_tarmac_actor_sample",
    "mdr_env_tarmac_actor_sample",
    "mdr_mlp_grad_floats", "mdr_mlp_grad_workspace_bytes", "mdr_ppo_actor_grad", "mdr_ppo_critic_grad", "mdr_dqn_target", "mdr_dqn_grad",
    "mdr_ppo_actor_grad_bf16x3", "mdr_ppo_critic_grad_bf16x3",
    "mdr_mappo_critic_grad_floats", "mdr_mappo_critic_workspace_bytes", "mdr_mappo_critic_grad",
    "mdr_mlp_wide_grad_floats", "mdr_mlp_wide_grad_workspace_bytes", "mdr_ppo_actor_grad_wide", "mdr_ppo_critic_grad_wide",
    "mdr_dqn_target_wide", "mdr_dqn_grad_wide",
    "mdr_mappo_critic_wide_grad_floats", "mdr_mappo_critic_wide_workspace_bytes", "mdr_mappo_critic_grad_wide",
    "mdr_maddpg_grad_floats", "mdr_maddpg_workspace_bytes", "mdr_maddpg_target", "mdr_maddpg_critic_grad", "mdr_maddpg_actor_grad",
    "mdr_mlp_actor_sample", "mdr_mlp_actor_sample_bf16x3", "mdr_mlp_actors_sample", "mdr_maddpg_target_agents",
    "mdr_env_mlp_actor_sample", "mdr_env_mlp_actor_sample_bf16x3",
    "mdr_maddpg_workspace_bytes_all", "mdr_maddpg_target_all", "mdr_maddpg_critic_grad_all", "mdr_maddpg_actor_grad_all",
    "mdr_tarmac_net_grad_floats", "mdr_tarmac_ppo_workspace_bytes", "mdr_tarmac_ppo_actor_grad", "mdr_tarmac_ppo_actor_grad_keyed",
    "mdr_tarmac_critic_grad_floats", "mdr_tarmac_critic_workspace_bytes", "mdr_tarmac_critic_value", "mdr_tarmac_critic_grad",
    "mdr_tarmac_a2c_grad_floats", "mdr_tarmac_a2c_workspace_bytes", "mdr_tarmac_a2c_forward", "mdr_tarmac_a2c_comm", "mdr_tarmac_a2c_grad",
    "mdr_adam_workspace_bytes", "mdr_adam_step", "mdr_adam_step_table", "mdr_adam_corrections",
    "mdr_adam_nets_table_bytes", "mdr_adam_nets_bind", "mdr_adam_step_nets",
    "mdr_minibatch_permutation", "mdr_minibatch_permutation_keyed", "mdr_minibatch_sample", "mdr_minibatch_sample_keyed",
    "mdr_update_cursor_set", "mdr_update_cursor_add", "mdr_maddpg_draws", "mdr_maddpg_draws_keyed",
)

_lib = None


class NativeLibraryMissing(RuntimeError):
    pass


def load():
    """dlopen the HIP library (once).  Raises NativeLibraryMissing if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise NativeLibraryMissing(
            "HIP library not built: %s is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64, libmdr_hip.so is linked against the
    # ones under /opt/rocm (same SONAMEs).  Whoever is loaded first is used by both; loaded the other way round - this library
    # first, torch afterwards - torch's HSA runtime comes up beside /opt/rocm's and the launches of this library fail with "no
    # ROCm-capable device is detected".  The host side owns its memory through torch anyway: bring torch's runtime in first.
    try:
        import torch  # noqa: F401
    except ImportError:      # a torch-free host (tools/c_abi_client.c is the C example) uses /opt/rocm's runtime alone
        pass
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u32, u64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64
    sig = {
        "mdr_abi_version": (C.c_int, []),
        "mdr_status_string": (C.c_char_p, [C.c_int]),
        "mdr_last_error": (C.c_char_p, [vp]),
        "mdr_partials_per_env": (i64, [i32]),
        "mdr_env_partial_records": (i64, [vp]),
        "mdr_env_create": (C.c_int, [C.POINTER(MdrConfig), C.POINTER(vp)]),
        "mdr_env_destroy": (C.c_int, [vp]),
        "mdr_env_bind": (C.c_int, [vp, C.POINTER(MdrBuffers)]),
        "mdr_env_reset": (C.c_int, [vp, u64, u32, vp]),
        "mdr_env_load_episode": (C.c_int, [vp, C.POINTER(MdrEpisode), u64, u32, vp]),
        "mdr_env_params_changed": (C.c_int, [vp, vp]),
        "mdr_env_bind_hvac_code": (C.c_int, [vp, vp, vp]),
        "mdr_env_bind_thermal_pack": (C.c_int, [vp, vp, vp]),
        "mdr_env_rollout_plan": (C.c_int, [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "mdr_env_rollout_resident": (C.c_int, [vp, C.POINTER(C.c_int32)]),
        "mdr_rollout_rows": (i64, [i32]),
        "mdr_env_bind_rollout_rows": (C.c_int, [vp, vp, i64]),
        "mdr_env_rollout_steps_per_launch": (C.c_int, [vp, C.POINTER(i64)]),
        "mdr_env_fill_rollout_rows": (C.c_int, [vp, i64, i32, vp, vp]),
        "mdr_env_set_od_table": (C.c_int, [vp, vp, i64]),
        "mdr_env_set_interp_grid": (C.c_int, [vp, C.POINTER(MdrInterpGrid)]),
        "mdr_env_begin_episode": (C.c_int, [vp, vp]),
        "mdr_env_refresh_obs": (C.c_int, [vp, vp]),
        "mdr_env_step": (C.c_int, [vp, vp, C.c_int, vp]),
        "mdr_env_rollout": (C.c_int, [vp, vp, C.c_int, i32, vp]),
        "mdr_env_rollout_fused": (C.c_int, [vp, vp, i32, C.POINTER(MdrRolloutOut), vp]),
        "mdr_env_set_controller": (C.c_int, [vp, C.c_int]),
        "mdr_env_greedy_myopic_actions": (C.c_int, [vp, vp, vp]),
        "mdr_env_step_begin": (C.c_int, [vp, vp, C.c_int, vp]),
        "mdr_env_step_end": (C.c_int, [vp, vp]),
        "mdr_env_step_end_gathered": (C.c_int, [vp, vp, i32, vp]),
        "mdr_env_step_begin_records": (C.c_int, [vp, vp, C.c_int, i32, vp]),
        "mdr_env_step_end_records": (C.c_int, [vp, vp, i32, vp]),
        "mdr_env_step_end_begin_records": (C.c_int, [vp, vp, i32, vp, C.c_int, vp]),
        "mdr_env_interp_due": (C.c_int, [vp]),
        "mdr_env_interp_local": (C.c_int, [vp, vp]),
        "mdr_env_interp_apply": (C.c_int, [vp, vp]),
        "mdr_obs_vector_length": (i32, [C.POINTER(MdrObsSpec)]),
        "mdr_env_obs_vector": (C.c_int, [vp, C.POINTER(MdrObsSpec), vp, vp]),
        "mdr_obs_message_fields": (i32, [C.POINTER(MdrObsSpec)]),
        "mdr_env_obs_messages": (C.c_int, [vp, C.POINTER(MdrObsSpec), vp, i64, vp]),
        "mdr_env_obs_vector_ext": (C.c_int, [vp, C.POINTER(MdrObsSpec), vp, i64, vp, vp]),
        "mdr_env_comm_draws": (C.c_int, [vp, C.POINTER(MdrObsSpec), vp, vp, vp]),
        "mdr_env_cursor": (C.c_int, [vp, C.POINTER(i64), C.POINTER(i64)]),
        "mdr_env_set_cursor": (C.c_int, [vp, u64, u32, i64, i64]),
        "mdr_env_active_tables": (C.c_int, [vp]),
        "mdr_actor_steps1": (i64, [i32, i32]),
        "mdr_actor_steps1_order": (i64, [i32, i32, i32]),
        "mdr_actor_steps2": (i64, [i32, i32]),
        "mdr_actor_frag1_floats": (i64, [i32, i32]),
        "mdr_actor_frag2_floats": (i64, [i32, i32]),
        "mdr_actor_sample": (C.c_int, [vp, vp, i64, i64, u64, u64, vp, vp, vp, vp, vp]),
        "mdr_env_actor_sample": (C.c_int, [vp, C.POINTER(MdrObsSpec), vp, u64, u64, vp, vp, vp, vp, vp, vp]),
        "mdr_env_actor_sample_links": (C.c_int, [vp, C.POINTER(MdrObsSpec), vp, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp]),
        "mdr_discounted_returns": (C.c_int, [vp, vp, vp, C.c_float, i32, i64, vp, vp]),
        "mdr_tarmac_comm": (C.c_int, [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, C.c_float, u64, u64, vp, i32, vp, i64, vp]),
        "mdr_logits_sample": (C.c_int, [vp, i64, i64, u64, u64, vp, i32, vp, vp, vp, vp]),
        "mdr_tarmac_comm_backward": (C.c_int, [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, C.c_float, u64, u64, vp, i32, vp, i64,
                                               vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]),
        "mdr_tarmac_comm_backward_workspace_bytes": (i64, [i64, i32, i32]),
        # the keyed siblings: a device int32 [2] key in place of the seed
        "mdr_tarmac_comm_keyed": (C.c_int, [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, C.c_float, vp, u64, vp, i32, vp, i64, vp]),
        "mdr_tarmac_comm_backward_keyed": (C.c_int, [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, C.c_float, vp, u64, vp, i32, vp,
                                                     i64, vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]),
        "mdr_tarmac_gather": (C.c_int, [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, u64, u64, vp, i32, vp, i64, vp]),
        "mdr_tarmac_gather_backward": (C.c_int, [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, i32, u64, u64, vp, i32, vp, i64,
                                                 vp, i64, vp, i64, vp, i64, vp, i64, vp, vp]),
        "mdr_tarmac_gather_backward_workspace_bytes": (i64, [i32, i32, i32, i32, i32, i32]),
        "mdr_tarmac_frag_encode_floats": (i64, [i32, i32]),
        "mdr_tarmac_frag_proj_floats": (i64, [i32, i32]),
        "mdr_tarmac_frag_msg_floats": (i64, [i32, i32]),
        "mdr_tarmac_frag_head_floats": (i64, [i32, i32, i32]),
        "mdr_tarmac_vec_floats": (i64, [i32, i32]),
        "mdr_tarmac_frag_words": (i64, [vp, i32]),
        "mdr_tarmac_actor_workspace_bytes": (i64, [vp, i64]),
        "mdr_tarmac_actor_sample": (C.c_int, [vp, vp, i32, i32, u64, u64, vp, vp, vp, vp, vp, vp]),
        "mdr_env_tarmac_actor_sample": (C.c_int, [vp, C.POINTER(MdrObsSpec), vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]),
        "mdr_mlp_grad_floats": (i64, [C.POINTER(MdrMlp)]),
        "mdr_mlp_grad_workspace_bytes": (i64, [C.POINTER(MdrMlp), i64, i32]),
        "mdr_ppo_actor_grad": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp]),
        "mdr_ppo_critic_grad": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mdr_ppo_actor_grad_bf16x3": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp]),
        "mdr_ppo_critic_grad_bf16x3": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mdr_dqn_target": (C.c_int, [C.POINTER(MdrMlp), C.POINTER(MdrMlp), vp, i64, vp, i64, vp, C.c_float, i32, vp, vp, vp, vp]),
        "mdr_dqn_grad": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp]),
        "mdr_mappo_critic_grad_floats": (i64, [C.POINTER(MdrMlp), i32]),
        "mdr_mappo_critic_workspace_bytes": (i64, [C.POINTER(MdrMlp), i32, i64, i32]),
        "mdr_mappo_critic_grad": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, i32, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp]),
        # the wide siblings (65..128 input features): the same argument lists
        "mdr_mlp_wide_grad_floats": (i64, [C.POINTER(MdrMlp)]),
        "mdr_mlp_wide_grad_workspace_bytes": (i64, [C.POINTER(MdrMlp), i64, i32]),
        "mdr_ppo_actor_grad_wide": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, vp, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp]),
        "mdr_ppo_critic_grad_wide": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mdr_dqn_target_wide": (C.c_int, [C.POINTER(MdrMlp), C.POINTER(MdrMlp), vp, i64, vp, i64, vp, C.c_float, i32, vp, vp, vp, vp]),
        "mdr_dqn_grad_wide": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, vp, vp, C.c_float, i32, vp, vp, vp, vp, vp]),
        "mdr_mappo_critic_wide_grad_floats": (i64, [C.POINTER(MdrMlp), i32]),
        "mdr_mappo_critic_wide_workspace_bytes": (i64, [C.POINTER(MdrMlp), i32, i64, i32]),
        "mdr_mappo_critic_grad_wide": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, i32, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp]),
        "mdr_maddpg_grad_floats": (i64, [C.POINTER(MdrMlp)]),
        "mdr_maddpg_workspace_bytes": (i64, [C.POINTER(MdrMlp), C.POINTER(MdrMlp), i32, i64, i32]),
        "mdr_maddpg_target": (C.c_int, [C.POINTER(MdrMlp), C.POINTER(MdrMlp), vp, i64, vp, vp, i64, i32, i32, vp, C.c_float, C.c_float, i32,
                                        vp, vp, vp, vp]),
        "mdr_maddpg_critic_grad": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, vp, i64, i32, vp, i32, vp, vp, vp, vp, vp]),
        "mdr_maddpg_actor_grad": (C.c_int, [C.POINTER(MdrMlp), C.POINTER(MdrMlp), vp, i64, vp, vp, i64, i32, i32, vp, C.c_float, C.c_float,
                                            i32, vp, vp, vp, vp, vp, vp]),
        "mdr_mlp_actor_sample": (C.c_int, [C.POINTER(MdrMlp), vp, i64, i64, u64, u64, vp, i32, i32, vp, vp, vp, vp]),
        "mdr_mlp_actor_sample_bf16x3": (C.c_int, [C.POINTER(MdrMlp), vp, i64, i64, u64, u64, vp, i32, i32, vp, vp, vp, vp]),
        "mdr_env_mlp_actor_sample": (C.c_int, [vp, C.POINTER(MdrObsSpec), C.POINTER(MdrMlp), u64, u64, vp, i32, i32, vp, vp, vp, vp, vp]),
        "mdr_env_mlp_actor_sample_bf16x3": (C.c_int, [vp, C.POINTER(MdrObsSpec), C.POINTER(MdrMlp), u64, u64, vp, i32, i32, vp, vp, vp, vp, vp]),
        # one net per agent: a host array of descriptors and its length in front
        "mdr_mlp_actors_sample": (C.c_int, [C.POINTER(MdrMlp), i32, vp, i64, i64, u64, u64, vp, i32, i32, vp, vp, vp, vp]),
        "mdr_maddpg_target_agents": (C.c_int, [C.POINTER(MdrMlp), i32, C.POINTER(MdrMlp), vp, i64, vp, vp, i64, i32, i32, vp, C.c_float,
                                               C.c_float, i32, vp, vp, vp, vp]),
        # all agents in one pass: host arrays of one descriptor per agent, no `agent` argument
        "mdr_maddpg_workspace_bytes_all": (i64, [C.POINTER(MdrMlp), C.POINTER(MdrMlp), i32, i64, i32]),
        "mdr_maddpg_target_all": (C.c_int, [C.POINTER(MdrMlp), C.POINTER(MdrMlp), vp, i64, vp, vp, i64, i32, vp, C.c_float, C.c_float, i32,
                                            vp, vp, vp, vp]),
        "mdr_maddpg_critic_grad_all": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, vp, i64, i32, vp, i32, vp, vp, vp, vp, vp]),
        "mdr_maddpg_actor_grad_all": (C.c_int, [C.POINTER(MdrMlp), C.POINTER(MdrMlp), vp, i64, vp, vp, i64, i32, vp, C.c_float, C.c_float,
                                                i32, vp, vp, vp, vp, vp, vp]),
        "mdr_tarmac_critic_grad_floats": (i64, [C.POINTER(MdrMlp)]),
        "mdr_tarmac_critic_workspace_bytes": (i64, [C.POINTER(MdrMlp), i64, i32]),
        "mdr_tarmac_critic_value": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, i64, i32, vp, vp]),
        "mdr_tarmac_critic_grad": (C.c_int, [C.POINTER(MdrMlp), vp, i64, vp, vp, i64, i32, vp, vp, vp, vp, vp, vp]),
        "mdr_tarmac_net_grad_floats": (i64, [C.POINTER(MdrTarmacNet)]),
        "mdr_tarmac_ppo_workspace_bytes": (i64, [C.POINTER(MdrTarmacNet), i64, i32, i32]),
        "mdr_tarmac_ppo_actor_grad": (C.c_int, [C.POINTER(MdrTarmacNet), vp, i64, vp, i64, i32, vp, vp, vp, C.c_float, u64, u64, i32, vp, vp, vp,
                                                vp, vp]),
        "mdr_tarmac_ppo_actor_grad_keyed": (C.c_int, [C.POINTER(MdrTarmacNet), vp, i64, vp, i64, i32, vp, vp, vp, C.c_float, vp, u64, vp, i32, vp,
                                                      vp, vp, vp, vp]),
        "mdr_tarmac_a2c_grad_floats": (i64, [C.POINTER(MdrTarmacA2CNet)]),
        "mdr_tarmac_a2c_workspace_bytes": (i64, [C.POINTER(MdrTarmacA2CNet), i64, i32, i32]),
        "mdr_tarmac_a2c_forward": (C.c_int, [C.POINTER(MdrTarmacA2CNet), vp, i64, vp, i64, vp, i64, i32, i32, vp, vp, vp, vp, vp]),
        "mdr_tarmac_a2c_comm": (C.c_int, [C.POINTER(MdrTarmacA2CNet), vp, i64, i32, i32, vp, i64, vp, vp]),
        "mdr_tarmac_a2c_grad": (C.c_int, [C.POINTER(MdrTarmacA2CNet), vp, i64, vp, i64, vp, vp, vp, i64, i32, C.c_float, C.c_float, i32, vp,
                                          vp, vp, vp, vp, vp]),
        "mdr_adam_workspace_bytes": (i64, [i64]),
        "mdr_adam_step": (C.c_int, [C.POINTER(MdrAdamSegments), vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, i64, C.c_double, C.c_double,
                                    C.c_double, vp, vp, i32, vp]),
        "mdr_adam_step_table": (C.c_int, [C.POINTER(MdrAdamSegments), vp, vp, C.c_double, C.c_double, C.c_double, C.c_double, vp, i32, vp,
                                          C.c_double, C.c_double, C.c_double, vp, vp, i32, vp]),
        "mdr_adam_corrections": (C.c_int, [C.c_double, C.c_double, C.c_double, i64, i64, vp]),
        "mdr_adam_nets_table_bytes": (i64, [i32]),
        "mdr_adam_nets_bind": (C.c_int, [vp, i32, C.POINTER(MdrAdamSegments), vp, vp, vp]),
        "mdr_adam_step_nets": (C.c_int, [vp, i32, i64, C.c_double, C.c_double, C.c_double, C.c_double, i64, C.c_double, C.c_double, C.c_double,
                                         vp, vp, vp]),
        "mdr_minibatch_permutation": (C.c_int, [i64, u64, u64, vp, vp, vp]),
        "mdr_minibatch_permutation_keyed": (C.c_int, [i64, vp, u64, vp, vp, vp]),
        "mdr_minibatch_sample": (C.c_int, [i64, vp, i64, u64, u64, vp, vp, vp]),
        "mdr_minibatch_sample_keyed": (C.c_int, [i64, vp, i64, vp, u64, vp, vp, vp]),
        "mdr_maddpg_draws": (C.c_int, [i32, i64, vp, i64, u64, u64, vp, vp, vp, vp, vp]),
        "mdr_maddpg_draws_keyed": (C.c_int, [i32, i64, vp, i64, vp, u64, vp, vp, vp, vp, vp]),
        "mdr_update_cursor_set": (C.c_int, [vp, i32, i32, i32, i32, i32, vp]),
        "mdr_update_cursor_add": (C.c_int, [vp, i32, i32, vp]),
        "mdr_env_pack": (C.c_int, [vp, i32, vp, vp]),
        "mdr_env_graph_room": (i64, [vp]),
        "mdr_env_graph_replayed": (C.c_int, [vp, i64, vp]),
        "mdr_mailbox_bytes": (i64, [i32, i32, i32]),
        "mdr_persist_records": (i64, [i32]),
        "mdr_env_rollout_persistent": (C.c_int, [vp, vp, i32, C.POINTER(MdrRolloutOut), C.POINTER(MdrMailbox), vp]),
        "mdr_mailbox_alloc": (C.c_int, [i64, i32, C.POINTER(vp)]),
        "mdr_mailbox_free": (C.c_int, [vp]),
        "mdr_mailbox_export": (C.c_int, [vp, C.c_char_p]),
        "mdr_mailbox_open": (C.c_int, [C.c_char_p, C.POINTER(vp)]),
        "mdr_mailbox_close": (C.c_int, [vp]),
        "mdr_mailbox_peek": (C.c_int, [vp, C.POINTER(u64)]),
        "mdr_env_step_mailbox": (C.c_int, [vp, vp, C.c_int, C.POINTER(MdrMailbox), u32, vp]),
        "mdr_mailbox_halo_bytes": (i64, [i32, i64]),
        "mdr_mailbox_halo_push": (C.c_int, [C.POINTER(MdrMailbox), i32, vp, i64, u32, vp]),
        "mdr_mailbox_halo_pull": (C.c_int, [C.POINTER(MdrMailbox), i32, vp, i64, u32, u32, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.mdr_abi_version() != MDR_ABI_VERSION:
        raise RuntimeError("libmdr_hip.so ABI version %d, binding expects %d" % (lib.mdr_abi_version(), MDR_ABI_VERSION))
    _lib = lib
    return lib


def check(lib, handle, rc, what):
    """Map a status code to the exception the reference would raise for the same condition."""
    if rc == MDR_OK:
        return
    msg = lib.mdr_last_error(handle).decode() if handle else ""
    text = "%s: %s%s" % (what, lib.mdr_status_string(rc).decode(), (" - " + msg) if msg else "")
    if rc == MDR_ERR_INVALID:
        raise ValueError(text)
    raise RuntimeError(text)
