"""ctypes mirror of include/lgx.h (the C-ABI of liblgx.so).

Everything Python repeats from the header is stated here once, in three tables: STRUCTS (the
structures, field for field), SIGS (every prototype) and CONSTANTS (every #define / enum value with
the Python value that mirrors it).  tests/test_abi_host.py compiles a probe against the header alone
and compares all three, offsets and argument widths included; `check_layout` is the load-time guard
against a stale library, from the library's own `lgx_struct_sizes`.
This module only describes the ABI; loading the product library is `legged_gym_amd.sim.lib`.
"""
import ctypes as C

NUM_DOF = 12
NUM_DYN = 13
MAX_BODIES = 17
MAX_POINTS = 128
MAX_OBS = 256
MAX_HEIGHT_POINTS = 192
MAX_TERMS = 24
ENV_BLOCK = 4    # smallest envs-per-workgroup the post-physics kernel is built with (sizes scratch)

# reward term ids (enum lgx_reward_term) keyed by the reference's `_reward_<name>` suffix
REWARD_IDS = {
    "lin_vel_z": 0, "ang_vel_xy": 1, "orientation": 2, "base_height": 3, "torques": 4, "energy": 5,
    "dof_vel": 6, "dof_acc": 7, "action_rate": 8, "collision": 9, "termination": 10,
    "dof_pos_limits": 11, "dof_vel_limits": 12, "torque_limits": 13, "tracking_lin_vel": 14,
    "tracking_ang_vel": 15, "feet_air_time": 16, "stumble": 17, "stand_still": 18,
    "feet_contact_forces": 19, "hip_motion": 20, "no_fly": 21,
}
CTRL = {"POS_DRIVE": 0, "P": 1, "V": 2, "T": 3, "SEA": 4}
# enum lgx_buffer_id in order: the state tensors lgx_sim_buffer reports; enum lgx_dtype in order,
# each with the name of its torch dtype
BUFFER_IDS = ("root_states", "dof_state", "dof_targets", "torques", "contact_forces", "actions",
              "last_actions", "last_dof_vel", "last_root_vel", "commands", "base_lin_vel", "base_ang_vel",
              "projected_gravity", "feet_air_time", "obs", "rew", "reset", "time_out", "episode_length",
              "episode_sums", "measured_heights", "env_origins", "terrain_levels", "terrain_types", "extras")
DTYPES = {"F32": "float32", "U8": "uint8", "I64": "int64"}

DRAW_CMD, DRAW_PUSH, DRAW_RESET_DOF, DRAW_RESET_XY = 0, 3, 5, 17
DRAW_RESET_VEL, DRAW_RESET_CMD, DRAW_CURRIC, DRAW_NOISE = 19, 25, 28, 32

f32, i32, i64, u64, vp = C.c_float, C.c_int32, C.c_int64, C.c_uint64, C.c_void_p
PF, PU8, PI64, PI16, PI32 = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int64), C.POINTER(C.c_int16), C.POINTER(C.c_int32)


class LgxModel(C.Structure):
    _fields_ = [
        ("joint_rot", f32 * 9 * NUM_DOF), ("joint_pos", f32 * 3 * NUM_DOF), ("joint_axis", f32 * 3 * NUM_DOF),
        ("dof_lower", f32 * NUM_DOF), ("dof_upper", f32 * NUM_DOF), ("dof_vel_limit", f32 * NUM_DOF),
        ("dof_effort", f32 * NUM_DOF), ("kp", f32 * NUM_DOF), ("kd", f32 * NUM_DOF),
        ("body_mass", f32 * NUM_DYN), ("body_com", f32 * 3 * NUM_DYN), ("body_inertia", f32 * 6 * NUM_DYN),
        ("num_points", i32), ("num_report_bodies", i32), ("leg_dof", i32), ("pad_model", i32),
        ("point_pos", f32 * 3 * MAX_POINTS), ("point_radius", f32 * MAX_POINTS),
        ("point_dyn", i32 * MAX_POINTS), ("point_report", i32 * MAX_POINTS),
        ("contact_k", f32), ("contact_c", f32), ("friction_c", f32), ("limit_k", f32), ("limit_c", f32),
        ("ground_friction", f32), ("gravity", f32 * 3), ("sim_dt", f32),
    ]


class LgxEnvParams(C.Structure):
    _fields_ = [
        ("num_envs", i32), ("num_obs", i32), ("decimation", i32), ("control_type", i32),
        ("action_scale", f32), ("clip_actions", f32), ("clip_obs", f32), ("dt", f32),
        ("default_dof_pos", f32 * NUM_DOF), ("soft_lower", f32 * NUM_DOF), ("soft_upper", f32 * NUM_DOF),
        ("dof_vel_limits", f32 * NUM_DOF), ("torque_limits", f32 * NUM_DOF),
        ("p_gains", f32 * NUM_DOF), ("d_gains", f32 * NUM_DOF),
        ("soft_dof_vel_limit", f32), ("soft_torque_limit", f32),
        ("max_episode_length", f32), ("max_episode_length_s", f32),
        ("resample_interval", i32), ("push_robots", i32), ("push_interval", i32), ("max_push_vel_xy", f32),
        ("heading_command", i32), ("cmd_ranges", f32 * 2 * 4),
        ("obs_scale_lin_vel", f32), ("obs_scale_ang_vel", f32), ("obs_scale_dof_pos", f32),
        ("obs_scale_dof_vel", f32), ("obs_scale_height", f32),
        ("add_noise", i32), ("noise_scale_vec", f32 * MAX_OBS),
        ("terrain_kind", i32), ("measure_heights", i32), ("num_height_points", i32),
        ("height_points", f32 * 2 * MAX_HEIGHT_POINTS),
        ("border_size", f32), ("horizontal_scale", f32), ("vertical_scale", f32),
        ("curriculum", i32), ("custom_origins", i32), ("max_terrain_level", i32), ("terrain_num_cols", i32),
        ("terrain_env_length", f32), ("base_init_state", f32 * 13),
        ("num_terms", i32), ("term_ids", i32 * MAX_TERMS), ("term_scales", f32 * MAX_TERMS),
        ("termination_slot", i32), ("termination_scale", f32), ("only_positive_rewards", i32),
        ("tracking_sigma", f32), ("base_height_target", f32), ("max_contact_force", f32),
        ("num_feet", i32), ("feet_indices", i32 * 4),
        ("num_penalised", i32), ("penalised_indices", i32 * 16),
        ("num_termination_bodies", i32), ("termination_indices", i32 * 8),
        ("send_timeouts", i32), ("use_actuator_history", i32),
        ("act_pos_err_mean", f32 * NUM_DOF), ("act_pos_err_std", f32 * NUM_DOF),
        ("act_vel_mean", f32 * NUM_DOF), ("act_vel_std", f32 * NUM_DOF),
        ("seed", u64),
    ]


BUFFER_FIELDS = [
    ("root_states", PF), ("dof_state", PF), ("dof_targets", PF), ("torques", PF), ("contact_forces", PF),
    ("actions", PF), ("last_actions", PF), ("last_dof_vel", PF), ("last_root_vel", PF), ("commands", PF),
    ("base_lin_vel", PF), ("base_ang_vel", PF), ("projected_gravity", PF), ("feet_air_time", PF),
    ("obs", PF), ("rew", PF), ("reset", PU8), ("time_out", PU8), ("episode_length", PI64),
    ("episode_sums", PF), ("measured_heights", PF), ("env_origins", PF), ("terrain_levels", PI64),
    ("terrain_types", PI64), ("terrain_origins", PF), ("height_samples", PI16), ("hf_rows", i32), ("hf_cols", i32),
    ("body_mass_scale", PF), ("friction", PF), ("act_hist", PF), ("model_ins", PF),
    ("act_net_w", PF), ("act_net_scale", PF), ("act_dvel", PF),
    ("extras", PF), ("extras_time_outs", PU8), ("scratch", PF),
    ("sea_w", PF), ("sea_h", PF), ("sea_c", PF), ("hf_trimesh", C.POINTER(C.c_int8)),
]


class LgxBuffers(C.Structure):
    _fields_ = BUFFER_FIELDS


class LgxMlpDesc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("rows", i64), ("nl", i32), ("act", i32), ("dims", i32 * 7),
                ("weights", C.c_void_p * 6), ("biases", C.c_void_p * 6)]


class LgxMlpX3Desc(C.Structure):
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("rows", i64), ("nl", i32), ("act", i32), ("dims", i32 * 7),
                ("weights", C.c_void_p * 6), ("biases", C.c_void_p * 6)]


class LgxPpoLossArgs(C.Structure):
    _fields_ = [("rows", i64), ("num_actions", i32), ("use_clipped_value_loss", i32), ("clip_param", C.c_float),
                ("value_loss_coef", C.c_float), ("entropy_coef", C.c_float)] + [
        (n, C.c_void_p) for n in ("idx", "mu_raw", "v_raw", "b4a", "b4c", "std", "actions", "old_logp", "old_mu",
                                  "old_sigma", "advantages", "target_values", "returns", "d_mu", "d_v", "partials",
                                  "g_std", "g_b4a", "g_b4c", "stats", "lr")] + [("desired_kl", C.c_double)] + [
        (n, C.c_void_p) for n in ("head_in", "W4a", "W4c")] + [("hidden", i32), ("defer_finalize", i32)]


class LgxReduceJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("n", i64), ("job_stride", i64), ("slice_stride", i64),
                ("dst_stride", i64), ("slices", i32), ("count", i32)]


class LgxPpoActArgs(C.Structure):
    _fields_ = [("num_envs", i64), ("num_actions", i32), ("num_obs", i32), ("num_cobs", i32), ("pad", i32)] + [
        (n, C.c_void_p) for n in ("mu", "value", "std", "noise", "obs", "cobs", "actions_out", "st_obs", "st_cobs",
                                  "st_actions", "st_values", "st_logp", "st_mu", "st_sigma")]


class LgxPpoStoreArgs(C.Structure):
    _fields_ = [("num_envs", i64), ("gamma", C.c_float), ("pad", i32)] + [
        (n, C.c_void_p) for n in ("rew", "reset", "time_outs", "st_values", "st_rew", "st_dones")]


class LgxGemmArgs(C.Structure):
    _fields_ = [("M", i64), ("N", i32), ("K", i32), ("batch", i32), ("epi", i32),
                ("A", C.c_void_p), ("lda", i64), ("sa", i64), ("B", C.c_void_p), ("ldb", i64), ("sb", i64),
                ("C", C.c_void_p), ("ldc", i64), ("sc", i64), ("bias", C.c_void_p), ("Y", C.c_void_p),
                ("partials", C.c_void_p), ("algo", i32), ("tile_rows", i32), ("Bs", C.c_void_p)]


class LgxGemmTnArgs(C.Structure):
    _fields_ = [("M", i64), ("R", i32), ("Cc", i32), ("slices", i32), ("batch", i32),
                ("A", C.c_void_p), ("lda", i64), ("sa", i64), ("B", C.c_void_p), ("ldb", i64), ("sb", i64),
                ("C", C.c_void_p), ("ldc", i64), ("colsum", C.c_void_p)]


class LgxCopy2dJob(C.Structure):
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("src_ld", i64), ("src_bs", i64), ("dst_ld", i64),
                ("dst_bs", i64), ("rows", i32), ("cols", i32), ("batch", i32), ("transpose", i32)]


MAX_PRIV_OBS = 512        # LGX_MAX_PRIV_OBS
PRIV_MAX_TERMS = 8        # LGX_PRIV_MAX_TERMS
# enum lgx_priv_term keyed by the names of cfg.privileged.terms (envs/base/privileged.py holds the widths)
PRIV_TERM_IDS = {"friction": 0, "base_mass": 1, "mass_scale": 2, "feet_contact": 3, "feet_forces": 4, "torques": 5}


class LgxPrivObsDesc(C.Structure):
    _fields_ = [("width", i32), ("num_terms", i32), ("term_ids", i32 * PRIV_MAX_TERMS),
                ("term_offsets", i32 * PRIV_MAX_TERMS), ("contact_force_scale", f32), ("torque_scale", f32)]


class LgxObsHistoryDesc(C.Structure):   # lgx_obs_history_desc (layout: envs/base/history.py)
    _fields_ = [("frames", i32), ("frame_width", i32), ("width", i32)]


class LgxActuatorRandDesc(C.Structure):   # lgx_actuator_rand_desc (the draws: envs/base/actuator_rand.py)
    _fields_ = [("kp_scale", C.c_void_p), ("kd_scale", C.c_void_p), ("lag", C.c_void_p)]


class LgxCmdCurriculumDesc(C.Structure):   # lgx_cmd_curriculum_desc (the rule: envs/base/command_curriculum.py)
    _fields_ = [("max_curriculum", f32), ("threshold", f32), ("state", C.c_void_p)]


class LgxObsNormJob(C.Structure):   # lgx_obs_norm_job (rl/normalizer.py)
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("rows", i64), ("width", i32), ("update", i32),
                ("parts", C.c_void_p), ("nparts", i64), ("state_in", C.c_void_p), ("state_out", C.c_void_p),
                ("eps", C.c_double)]


class LgxSymmetryArgs(C.Structure):   # lgx_symmetry_args (the tables: envs/base/symmetry.py)
    _fields_ = [("rows", i64), ("src_row", i64), ("dst_row", i64),
                ("num_obs", i32), ("num_cobs", i32), ("num_actions", i32), ("pad", i32)] + [
        (n, C.c_void_p) for n in ("observations", "privileged_observations", "actions", "mu", "sigma",
                                  "actions_log_prob", "advantages", "values", "returns", "obs_perm", "obs_sign",
                                  "cobs_perm", "cobs_sign", "act_perm", "act_sign")]


OBS_NORM_ROWS = 64       # LGX_OBS_NORM_ROWS (checked against lgx_obs_norm_rows_per_part at first use)
OBS_NORM_MAX_JOBS = 2     # LGX_OBS_NORM_MAX_JOBS
PPO_MAX_ACTIONS = 16
MAX_REDUCE_JOBS = 16
EPISODE_RING_MAX = 4096   # LGX_EPISODE_RING_MAX: largest ring of lgx_episode_stats_step
COMM_ID_BYTES = 128       # LGX_COMM_ID_BYTES: the unique id of lgx_comm_unique_id / lgx_comm_create
GEMM_PLAIN, GEMM_BIAS_ELU, GEMM_DELU_COLSUM, GEMM_DELU = 0, 1, 2, 3
GEMM_ALGO_DEFAULT, GEMM_ALGO_F32, GEMM_ALGO_SPLIT_BF16 = 0, 1, 2
GEMM_TILE_M, GEMM_TILE_N, GEMM_K_STEP = 128, 128, 32   # K step: layer-1 rows padded to 1024 B (aligned 128-B lines)


# Every prototype of lgx.h as (restype, argtypes), keyed by the name after the library's prefix: the
# entry points the CPU oracle shares in form, then the product library's own.  `declare` attaches
# them, EXPORTED is their names, and tests/test_abi_host.py checks each against the header.
SIGS_COMMON = {
    "last_error": (C.c_char_p, []),
    "version": (C.c_int, []),
    "struct_sizes": (None, [C.POINTER(C.c_int64)]),
    "scratch_floats": (C.c_int64, [i32, i32]),
    "sim_create": (C.c_int, [C.POINTER(LgxModel), C.POINTER(LgxEnvParams), C.POINTER(LgxBuffers), C.c_int,
                             C.POINTER(vp)]),
    "sim_destroy": (C.c_int, [vp]),
    "step": (C.c_int, [vp, i64, vp]),
    "simulate": (C.c_int, [vp, i32, vp]),
    "post_physics": (C.c_int, [vp, i64, vp]),
    "post_physics_fused": (C.c_int, [vp, i64, vp]),
    "reset_idx": (C.c_int, [vp, vp, i32, i64, i32, vp]),
    "set_draws": (C.c_int, [vp, vp]),
    "rebind_obs": (C.c_int, [vp, vp]),
    "actuator_mlp": (C.c_int, [vp, vp, i64, vp, vp, vp]),
    "actuator_lstm": (C.c_int, [vp, vp, vp, vp, i64, vp, vp]),
    "mlp_forward": (C.c_int, [vp, vp, i64, i32, C.POINTER(i32), C.POINTER(vp), C.POINTER(vp), i32, vp]),
    "gae": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, vp]),
    "gae_norm_scratch": (i64, [i32]),
    "gae_norm": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, vp, vp]),
    "gae_parts": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, vp, vp]),
    "adv_norm": (C.c_int, [vp, i64, vp, i32, vp]),
    "profile_enable": (C.c_int, [vp, i32]),
    "mlp_forward_batch": (C.c_int, [C.POINTER(LgxMlpDesc), i32, vp]),
    "profile_collect": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
}
SIGS_PRODUCT = {  # PPO update entry points and the later features: product library only
    "physics_lane_split": (i32, [i32]),
    "trimesh_build": (C.c_int, [vp, i32, i32, C.c_double, C.c_double, C.c_double, vp, vp, vp, vp]),
    "step_from": (C.c_int, [vp, vp, i64, vp]),
    "drive_inputs": (C.c_int, [vp, vp, vp]),
    "ground_contact": (C.c_int, [vp, vp, i32, vp, vp]),
    "sync_aux": (C.c_int, [vp, vp]),
    "rebind_extras": (C.c_int, [vp, vp]),
    "bind_privileged_obs": (C.c_int, [vp, vp, C.POINTER(LgxPrivObsDesc)]),
    "rebind_privileged_obs": (C.c_int, [vp, vp]),
    "bind_obs_history": (C.c_int, [vp, vp, vp, C.POINTER(LgxObsHistoryDesc)]),
    "rebind_obs_history": (C.c_int, [vp, vp, vp]),
    "bind_actuator_rand": (C.c_int, [vp, C.POINTER(LgxActuatorRandDesc)]),
    "bind_command_curriculum": (C.c_int, [vp, C.POINTER(LgxCmdCurriculumDesc)]),
    "is_curriculum_step": (i32, [i64, C.c_float]),
    "set_command_range": (C.c_int, [vp, i32, C.c_float, C.c_float, vp]),
    "sim_buffer": (C.c_int, [vp, i32, C.POINTER(vp), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]),
    "ppo_gather_rows": (C.c_int, [vp, vp, vp, i64, i32, vp]),
    "ppo_act": (C.c_int, [C.POINTER(LgxPpoActArgs), vp]),
    "ppo_store": (C.c_int, [C.POINTER(LgxPpoStoreArgs), vp]),
    "ppo_act_store": (C.c_int, [C.POINTER(LgxPpoActArgs), C.POINTER(LgxPpoStoreArgs), vp]),
    "bias_act": (C.c_int, [vp, vp, i64, i32, i32, i32, vp]),
    "ppo_loss_partials_floats": (i64, [i64, i32]),
    "ppo_loss": (C.c_int, [C.POINTER(LgxPpoLossArgs), vp]),
    "ppo_adapt_lr": (C.c_int, [vp, C.c_float, vp, C.c_double, vp]),
    "head_bwd_partials_floats": (i64, [i64, i32, i32]),
    "head_bwd": (C.c_int, [vp, vp, vp, vp, vp, i64, i32, i32, vp, vp]),
    "head_bwd_finalize": (C.c_int, [C.POINTER(LgxPpoLossArgs), vp, vp, vp, vp, vp, i64, i32, i32, vp, vp]),
    "colsum_partials_floats": (i64, [i64, i32, i32]),
    "elu_bwd_colsum": (C.c_int, [vp, vp, i64, i32, i32, vp, vp]),
    "reduce_slices": (C.c_int, [C.POINTER(LgxReduceJob), i32, vp]),
    "reduce_slices_finalize": (C.c_int, [C.POINTER(LgxReduceJob), i32, C.POINTER(LgxPpoLossArgs), vp]),
    "reduce_slices_blocks": (i64, [C.POINTER(LgxReduceJob), i32, i32]),
    "reduce_slices_sq": (C.c_int, [C.POINTER(LgxReduceJob), i32, C.POINTER(LgxPpoLossArgs), vp, vp, vp]),
    "ppo_loss_bwd_layout": (C.c_int, [i64, i32, i32, C.POINTER(i64)]),
    "ppo_loss_bwd": (C.c_int, [C.POINTER(LgxPpoLossArgs), vp, vp]),
    "mlp_x3_weight_elems": (i64, [i32, i32]),
    "mlp_x3_split": (C.c_int, [vp, i32, i32, vp, vp]),
    "mlp_x3_split_layers": (C.c_int, [C.POINTER(vp), C.POINTER(i32), i32, C.POINTER(vp), vp]),
    "mlp_x3_lds_bytes": (i64, [C.POINTER(LgxMlpX3Desc), i32]),
    "mlp_x3_forward": (C.c_int, [C.POINTER(LgxMlpX3Desc), i32, vp]),
    "mlp_x3_forward_act": (C.c_int, [C.POINTER(LgxMlpX3Desc), i32, C.POINTER(LgxPpoActArgs),
                                     C.POINTER(LgxPpoStoreArgs), vp]),
    "gemm_partials_floats": (i64, [i64, i32, i32]),
    "gemm_nt": (C.c_int, [C.POINTER(LgxGemmArgs), vp]),
    "gemm_tn": (C.c_int, [C.POINTER(LgxGemmTnArgs), vp]),
    "copy2d": (C.c_int, [C.POINTER(LgxCopy2dJob), i32, vp]),
    "split_bf16_elems": (i64, [i32, i32]),
    "split_bf16": (C.c_int, [C.POINTER(LgxCopy2dJob), i32, vp]),
    "ppo_gather_rows_padded": (C.c_int, [vp, vp, vp, i64, i32, i32, vp]),
    "ppo_gather_rows_padded_dup": (C.c_int, [vp, vp, vp, i64, i32, i32, i64, vp]),
    "adam_clip": (C.c_int, [vp, vp, vp, vp, i64, vp, i32, C.c_float, C.c_float, vp, vp, C.c_float,
                            C.c_float, C.c_float, vp]),
    "adam_clip_mirror": (C.c_int, [vp, vp, vp, vp, i64, vp, i32, C.c_float, C.c_float, vp, vp, C.c_float,
                                   C.c_float, C.c_float, C.POINTER(LgxCopy2dJob), i32, vp]),
    "adam_clip_mirror_sq": (C.c_int, [vp, vp, vp, vp, i64, vp, i32, C.c_float, vp, vp, C.c_float,
                                      C.c_float, C.c_float, C.POINTER(LgxCopy2dJob), i32, vp]),
    "event_create": (C.c_int, [C.POINTER(vp)]),
    "event_destroy": (C.c_int, [vp]),
    "event_record": (C.c_int, [vp, vp]),
    "stream_wait_event": (C.c_int, [vp, vp]),
    "launch_bind_event": (C.c_int, [vp]),
    "launch_bind_pending": (C.c_int, []),
    "comm_unique_id": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint8)]),
    "comm_create": (C.c_int, [C.c_char_p, C.POINTER(C.c_uint8), i32, i32, i32, C.POINTER(vp)]),
    "comm_destroy": (C.c_int, [vp]),
    "allreduce_grads": (C.c_int, [vp, vp, C.c_size_t, i32, vp]),
    "episode_stats_step": (C.c_int, [vp, vp, i64, vp, vp, vp, vp, i32, vp, vp]),
    "obs_norm_rows_per_part": (i32, []),
    "obs_norm_part_doubles": (i64, [i64, i32]),
    "obs_norm_partials": (C.c_int, [C.POINTER(LgxObsNormJob), i32, vp]),
    "obs_norm_apply": (C.c_int, [C.POINTER(LgxObsNormJob), i32, vp]),
    "ppo_symmetry_augment": (C.c_int, [C.POINTER(LgxSymmetryArgs), vp]),
    "ppo_symmetry_check_table": (C.c_int, [vp, vp, i32]),
    "ppo_loss_bwd_mirror": (C.c_int, [C.POINTER(LgxPpoLossArgs), vp, vp, C.c_float, i64, vp, vp, vp]),
    "ppo_mirror_partials_floats": (i64, [i64]),
    "ppo_mirror_loss_reduce": (C.c_int, [vp, i64, C.c_float, vp, vp]),
    "bc_loss_bwd_layout": (C.c_int, [i64, i32, i32, C.POINTER(i64)]),
    "bc_loss_bwd": (C.c_int, [vp, vp, vp, vp, i64, i32, i32, C.c_float, vp, vp, vp]),
    "bc_loss_reduce": (C.c_int, [vp, i64, C.c_float, vp, vp]),
}
SIGS = {**SIGS_COMMON, **SIGS_PRODUCT}
EXPORTED = [f"lgx_{name}" for name in SIGS]


def declare(lib, prefix="lgx"):
    """Attach argtypes/restypes of the product C-ABI to a loaded CDLL."""
    for name, (res, args) in (SIGS if prefix == "lgx" else SIGS_COMMON).items():
        fn = getattr(lib, f"{prefix}_{name}")
        fn.restype = res
        fn.argtypes = args
    return lib


# The ABI structures with their C names; the first 12 in lgx_struct_sizes order.
STRUCTS = [
    (LgxModel, "lgx_model"), (LgxEnvParams, "lgx_env_params"), (LgxBuffers, "lgx_buffers"),
    (LgxMlpDesc, "lgx_mlp_desc"), (LgxPpoLossArgs, "lgx_ppo_loss_args"), (LgxReduceJob, "lgx_reduce_job"),
    (LgxPpoActArgs, "lgx_ppo_act_args"), (LgxPpoStoreArgs, "lgx_ppo_store_args"), (LgxGemmArgs, "lgx_gemm_args"),
    (LgxCopy2dJob, "lgx_copy2d_job"), (LgxGemmTnArgs, "lgx_gemm_tn_args"), (LgxMlpX3Desc, "lgx_mlp_x3_desc"),
    (LgxPrivObsDesc, "lgx_priv_obs_desc"), (LgxObsHistoryDesc, "lgx_obs_history_desc"),
    (LgxActuatorRandDesc, "lgx_actuator_rand_desc"), (LgxCmdCurriculumDesc, "lgx_cmd_curriculum_desc"),
    (LgxObsNormJob, "lgx_obs_norm_job"), (LgxSymmetryArgs, "lgx_symmetry_args"),
]

# C identifier -> the Python value that mirrors it, for every constant of lgx.h repeated above
CONSTANTS = {
    "LGX_NUM_DOF": NUM_DOF, "LGX_NUM_DYN": NUM_DYN, "LGX_MAX_BODIES": MAX_BODIES, "LGX_MAX_POINTS": MAX_POINTS,
    "LGX_MAX_OBS": MAX_OBS, "LGX_MAX_HEIGHT_POINTS": MAX_HEIGHT_POINTS, "LGX_MAX_TERMS": MAX_TERMS,
    **{f"LGX_R_{k.upper()}": v for k, v in REWARD_IDS.items()}, "LGX_R_COUNT": len(REWARD_IDS),
    **{f"LGX_CTRL_{k}": v for k, v in CTRL.items()},
    "LGX_DRAW_CMD": DRAW_CMD, "LGX_DRAW_PUSH": DRAW_PUSH, "LGX_DRAW_RESET_DOF": DRAW_RESET_DOF,
    "LGX_DRAW_RESET_XY": DRAW_RESET_XY, "LGX_DRAW_RESET_VEL": DRAW_RESET_VEL, "LGX_DRAW_RESET_CMD": DRAW_RESET_CMD,
    "LGX_DRAW_CURRIC": DRAW_CURRIC, "LGX_DRAW_NOISE": DRAW_NOISE,
    **{f"LGX_PRIV_{k.upper()}": v for k, v in PRIV_TERM_IDS.items()}, "LGX_PRIV_COUNT": len(PRIV_TERM_IDS),
    "LGX_MAX_PRIV_OBS": MAX_PRIV_OBS, "LGX_PRIV_MAX_TERMS": PRIV_MAX_TERMS,
    "LGX_OBS_NORM_ROWS": OBS_NORM_ROWS, "LGX_OBS_NORM_MAX_JOBS": OBS_NORM_MAX_JOBS,
    "LGX_PPO_MAX_ACTIONS": PPO_MAX_ACTIONS, "LGX_MAX_REDUCE_JOBS": MAX_REDUCE_JOBS,
    "LGX_EPISODE_RING_MAX": EPISODE_RING_MAX, "LGX_COMM_ID_BYTES": COMM_ID_BYTES,
    "LGX_GEMM_PLAIN": GEMM_PLAIN, "LGX_GEMM_BIAS_ELU": GEMM_BIAS_ELU, "LGX_GEMM_DELU_COLSUM": GEMM_DELU_COLSUM,
    "LGX_GEMM_DELU": GEMM_DELU, "LGX_GEMM_ALGO_DEFAULT": GEMM_ALGO_DEFAULT, "LGX_GEMM_ALGO_F32": GEMM_ALGO_F32,
    "LGX_GEMM_ALGO_SPLIT_BF16": GEMM_ALGO_SPLIT_BF16,
    **{f"LGX_BUF_{k.upper()}": v for v, k in enumerate(BUFFER_IDS)}, "LGX_BUF_COUNT": len(BUFFER_IDS),
    **{f"LGX_{k}": v for v, k in enumerate(DTYPES)},
}


def check_layout(sizes_fn, n=12):
    """Compare the library's sizeof() of the first n ABI structs with these mirrors (the oracle
    reports the first 3)."""
    out = (C.c_int64 * 16)()
    sizes_fn(out)
    mine = tuple(C.sizeof(cls) for cls, _ in STRUCTS[:n])
    if tuple(out)[:n] != mine:
        raise RuntimeError(f"lgx ABI layout mismatch: library {tuple(out)[:n]} vs bindings {mine}")
