"""ctypes binding of libcrl_hip.so (include/crl.h).  There is NO fallback: if the HIP
library is missing or fails to load, importing the backend raises."""
import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
# CRL_LIB_VARIANT=<tag>: a profiling build made by `python -m competitive_rl_amd.build --variant <tag> <flags>` (e.g. -DCRL_ABLATION:
# the bit-exact alternative kernels that tests A/B against the shipped ones); unset = the shipped library
LIB_PATH = os.path.join(PKG, "libcrl_hip_%s.so" % os.environ["CRL_LIB_VARIANT"] if os.environ.get("CRL_LIB_VARIANT") else "libcrl_hip.so")

CRL_ENV_PONG_DOUBLE, CRL_ENV_CAR_DOUBLE, CRL_ENV_PONG_SINGLE, CRL_ENV_CAR_SINGLE = 1, 2, 3, 4
CRL_FLAG_STACK_REPLICATE = 1
CAR_MAX_TILES = 512
CAR_MAP_ORG, CAR_MAP_W = 4392, 1216  # include/crl.h CRL_CAR_MAP_*
CRL_OBS_RAW_RGB, CRL_OBS_GRAY_RESIZED = 0, 1
PONG_FRAME_BYTES = 210 * 160 * 3
ATLAS_BYTES = 22 * 22 * 34 * 160

CRL_LEAGUE_MAX_AGENTS = 16
CRL_LEAGUE_RANDOM, CRL_LEAGUE_RULE_BASED, CRL_LEAGUE_LIGHT = 0, 1, 2
CRL_POOL_KIND_FULL = 3  # a full-size ActorCritic agent (crl_pool_add_full); a #define beside enum crl_league_kind
CRL_LEAGUE_DOMAIN_OPPONENT, CRL_LEAGUE_DOMAIN_ACTION, CRL_LEAGUE_DOMAIN_SAMPLE = 0x4C47554F, 0x4C475541, 0x4C475553
CRL_LEDGER_DOMAIN_OPPONENT = 0x4C475557
CRL_LEDGER_COUNTERS = 6  # rows of the counters tensor, in this order (enum crl_ledger_counter)
CRL_LEDGER_COUNTER_NAMES = ("episodes", "wins", "losses", "draws", "return_sum", "length_sum")
CRL_LEDGER_PFSP_HARD, CRL_LEDGER_PFSP_VARIANCE = 0, 1
CRL_ARENA_DOMAIN_PAIR = 0x4C475550
CRL_CAR_DRIVER_DOMAIN = 0x43524430  # "CRD0": car c draws under CRL_CAR_DRIVER_DOMAIN + c (include/crl.h "car drivers")
CRL_CAR_DRIVER_RANDOM, CRL_CAR_DRIVER_RULE_BASED = 0, 1
CRL_CAR_DRIVER_SLOTS = 16
CRL_CAR_POLICY_DOMAIN = 0x43525030  # "CRP0": car c draws under CRL_CAR_POLICY_DOMAIN + c (include/crl.h "car policy")
CRL_CAR_POLICY_SLOTS, CRL_CAR_OBS_FEATURES, CRL_CAR_POLICY_HIDDEN, CRL_CAR_POLICY_BLOB_FLOATS = 8, 21, 100, 2508
CRL_CAR_LEAGUE_DOMAIN = 0x43524C47  # "CRLG" (include/crl.h "car league")
CRL_CAR_LEAGUE_COUNTERS = 7  # planes of the counters tensor, in this order (enum crl_car_league_counter)
CRL_CAR_LEAGUE_COUNTER_NAMES = ("episodes", "wins", "losses", "draws", "return_sum", "opponent_return_sum", "length_sum")
CRL_CAR_LEAGUE_NETWORK, CRL_CAR_LEAGUE_STYLE = 0, 1
CRL_ARENA_COUNTERS = 6  # planes of the counters tensor, in this order (enum crl_arena_counter); each plane is [left][right]
CRL_ARENA_COUNTER_NAMES = ("episodes", "left_wins", "right_wins", "draws", "return_sum", "length_sum")

FRAME_DT = np.dtype([("ball_x", "<i2"), ("ball_y", "<i2"), ("bat_l_y", "u1"), ("bat_r_y", "u1"),
                     ("score_l", "u1"), ("score_r", "u1")])
STATE_DT = np.dtype([
    ("speed_x", "<f8"), ("speed_y", "<f8"), ("ball_x", "<i4"), ("ball_y", "<i4"),
    ("bat_l_y", "<i4"), ("bat_r_y", "<i4"), ("score_l", "<i4"), ("score_r", "<i4"),
    ("num_rounds", "<i4"), ("num_steps", "<i4"), ("serve_ctr", "<u4"), ("wrap_steps", "<i4"),
    ("keep", FRAME_DT, (2,)), ("hist", FRAME_DT, (3, 2)),
])


CAR_BODY_DT = np.dtype([(k, "<f4") for k in ("cx", "cy", "a", "vx", "vy", "w")])
CAR_STATE_DT = np.dtype([
    ("hull", CAR_BODY_DT), ("wheel", CAR_BODY_DT, (4,)), ("imp", "<f4", (4, 3)), ("motor_imp", "<f4", (4,)),
    ("motor_speed", "<f4", (4,)), ("limit_state", "<i4", (4,)), ("gas", "<f8", (4,)), ("omega", "<f8", (4,)), ("phase", "<f8", (4,)),
    ("reward", "<f8"), ("prev_reward", "<f8"), ("tile_visited_count", "<i4"), ("last_block", "<i4"), ("done", "<i4"),
    ("step_count", "<i4"), ("first_step", "<i4"), ("pad", "<i4"),
    ("wheel_tiles", "<u4", (4, CAR_MAX_TILES // 32)), ("visited", "<u4", (CAR_MAX_TILES // 32,)),
    ("sleep_time", "<f4", (5,)), ("pad2", "<f4")], align=True)
CAR_CONTACT_DT = np.dtype([("pair", "<i4"), ("count", "<i4"), ("type", "<i4"), ("ln", "<f4", (2,)), ("lp", "<f4", (2,)),
                           ("pt", "<f4", (2, 2)), ("id", "<u4", (2,)), ("nimp", "<f4", (2,)), ("timp", "<f4", (2,))])
CAR_ENV_STATE_DT = np.dtype([("car", CAR_STATE_DT, (2,)), ("elapsed", "<i4"), ("episode", "<u4"), ("n_contact", "<i4"), ("coupled", "<i4"),
                             ("contact", CAR_CONTACT_DT, (8,))], align=True)
CRL_FLAG_CAR_NO_CONTACTS = 2
CRL_FLAG_CAR_FMA = 4
CRL_CAR_DONE_ANY, CRL_CAR_DONE_CAR0 = 0, 1
CRL_OBS_U8, CRL_OBS_F32, CRL_OBS_F32_REF = 0, 1, 2
CRL_EACTION = -5


class CrlOpts(C.Structure):
    _fields_ = [("env_kind", C.c_int32), ("obs_mode", C.c_int32), ("resized_dim", C.c_int32),
                ("frame_stack", C.c_int32), ("num_envs", C.c_int64), ("env_id_base", C.c_int64),
                ("seed", C.c_uint64), ("device", C.c_int32), ("flags", C.c_int32), ("action_repeat", C.c_int32),
                ("done_policy", C.c_int32), ("obs_dtype", C.c_int32), ("reserved", C.c_int32)]


class CrlPpoHyper(C.Structure):
    """crl_ppo_hyper (include/crl.h "ppo update")."""
    _fields_ = [(k, C.c_float) for k in ("clip", "vf_coef", "ent_coef", "lr", "beta1", "beta2", "eps", "max_grad_norm")]


class CrlPpoTeacher(C.Structure):
    """crl_ppo_teacher (include/crl.h "ppo update, teacher targets")."""
    _fields_ = [("logits_dev", C.c_void_p), ("labels_dev", C.c_void_p), ("value_targets_dev", C.c_void_p), ("rows", C.c_int64),
                ("temperature", C.c_float), ("coef", C.c_float), ("policy_term", C.c_int32)]


class CrlCarPpoTeacher(C.Structure):
    """crl_car_ppo_teacher (include/crl.h "car ppo update, teacher targets")."""
    _fields_ = [("target_dev", C.c_void_p), ("value_targets_dev", C.c_void_p), ("rows", C.c_int64), ("teacher_log_std", C.c_float * 2),
                ("point", C.c_int32), ("kind", C.c_int32), ("coef", C.c_float), ("policy_term", C.c_int32)]


CRL_CAR_TEACHER_CE, CRL_CAR_TEACHER_MSE = 0, 1  # enum crl_car_teacher_kind


class CrlStackDesc(C.Structure):
    """crl_stack_desc (include/crl.h): a FrameStackTensor drawn by the step."""
    _fields_ = [("stack_dev", C.c_void_p), ("planes", C.c_int32), ("dtype", C.c_int32), ("agent", C.c_int32),
                ("valid_planes", C.c_int32), ("alias_newest", C.c_int32), ("reserved", C.c_int32)]


vp, i64, u64, i32, u32, f64, cstr, P = C.c_void_p, C.c_int64, C.c_uint64, C.c_int32, C.c_uint32, C.c_double, C.c_char_p, C.POINTER
f32 = C.c_float
# every symbol include/crl.h declares -> (restype, argtypes); load() applies it, tests check the library exports all of them
SIGNATURES = {
    "crl_create": (i32, [P(CrlOpts), vp, P(vp)]),
    "crl_destroy": (None, [vp]),
    "crl_seed": (i32, [vp, u64]),
    "crl_reset": (i32, [vp, vp, vp]),
    "crl_step": (i32, [vp, vp, vp, vp, vp, vp]),
    "crl_render": (i32, [vp, vp, vp]),
    "crl_info": (i32, [vp, P(vp), P(vp)]),
    "crl_copy_info": (i32, [vp, vp, vp, vp]),
    "crl_terminal_observation": (i32, [vp, vp, i64, vp, vp]),
    "crl_get_state": (i32, [vp, vp, i64, i64, vp]),
    "crl_set_state": (i32, [vp, vp, i64, i64, vp]),
    "crl_set_replay": (i32, [vp, vp, vp, vp, i64]),
    "crl_render_raw": (i32, [vp, vp, i64, vp, vp]),
    "crl_obs_bytes_per_env": (i64, [vp]),
    "crl_kernel_timing": (i32, [vp, i32]),
    "crl_kernel_time_ms": (i32, [vp, i32, P(f64), P(i64)]),
    "crl_last_error": (cstr, []),
    "crl_version": (cstr, []),
    "crl_car_get_state": (i32, [vp, vp, i64, i64, vp]),
    "crl_car_set_state": (i32, [vp, vp, i64, i64, vp]),
    "crl_car_get_track": (i32, [vp, i64, vp, vp, vp, vp, vp, vp]),
    "crl_car_set_track": (i32, [vp, i64, i32, vp, vp, vp, vp, vp]),
    "crl_car_get_map": (i32, [vp, i64, vp, vp, vp]),
    "crl_car_set_replay": (i32, [vp, vp, vp, i64]),
    "crl_policy_create": (i32, [i32, i64, vp, vp, vp, vp, vp, vp, P(vp)]),
    "crl_policy_create_full": (i32, [i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, P(vp)]),
    "crl_policy_destroy": (None, [vp]),
    "crl_policy_reset": (i32, [vp, vp]),
    "crl_policy_act": (i32, [vp, vp, i64, vp, i64, vp, vp]),
    "crl_policy_get_stack": (i32, [vp, vp, vp]),
    "crl_policy_set_stack": (i32, [vp, vp, vp]),
    "crl_policy_set_sampling": (i32, [vp, f32, f32, u64, i64]),
    "crl_policy_set_critic": (i32, [vp, vp, vp]),
    "crl_policy_act_rollout": (i32, [vp, vp, i64, vp, vp, i64, vp, vp, vp, vp]),
    "crl_policy_load_weights": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_terminal_observation_dev": (i32, [vp, vp, i64, vp, vp]),
    "crl_check": (i32, [vp, vp]),
    "crl_car_info": (i32, [vp, P(vp), P(vp)]),
    "crl_car_copy_info": (i32, [vp, vp, vp, vp, vp]),
    "crl_frame_stack_update": (i32, [vp, vp, i32, i64, vp, i64, i32, i32, i64, vp]),
    "crl_frame_stack_update_to": (i32, [vp, vp, vp, i32, i64, vp, i64, i32, i32, i64, vp]),
    "crl_frame_stack_update_u8": (i32, [vp, vp, vp, i32, i64, vp, i64, i32, i32, i64, vp]),
    "crl_ctx_last_error": (cstr, [vp]),
    "crl_obs_descriptors": (i32, [vp, vp, vp]),
    "crl_render_frames_dev": (i32, [vp, vp, i64, vp, vp]),
    "crl_car_cap_hits": (i32, [vp, vp, vp]),
    "crl_selftest_sincosf": (i32, [i32, u64, u64, vp]),
    "crl_step_stack": (i32, [vp, vp, vp, vp, vp, P(CrlStackDesc), vp]),
    "crl_draw_stack": (i32, [vp, vp, P(CrlStackDesc), vp]),
    "crl_set_flags_event": (i32, [vp, vp]),
    "crl_kernel_time_stats": (i32, [vp, i32, P(f64), P(i64), P(f64)]),
    "crl_draw_raw_delta": (i32, [vp, vp, vp, i32, vp]),
    "crl_step_raw_delta": (i32, [vp, vp, vp, vp, vp, vp, vp]),
    "crl_league_create": (i32, [i32, i64, i64, u64, P(vp)]),
    "crl_league_destroy": (None, [vp]),
    "crl_league_add_builtin": (i32, [vp, i32]),
    "crl_league_add_light": (i32, [vp, vp, vp, vp, vp, vp, vp]),
    "crl_pool_add_full": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, i64]),
    "crl_pool_load_light": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
    "crl_pool_load_full": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_sampling_set_agent": (i32, [vp, i32, f32, f32]),
    "crl_sampling_get_agent": (i32, [vp, i32, P(f32), P(f32)]),
    "crl_league_seed": (i32, [vp, u64, vp]),
    "crl_league_set_assignment": (i32, [vp, vp, i32, vp]),
    "crl_league_get_assignment": (i32, [vp, vp, vp]),
    "crl_league_resample": (i32, [vp, vp, vp]),
    "crl_league_get_lists": (i32, [vp, vp, vp, vp]),
    "crl_league_act": (i32, [vp, vp, i64, vp, i64, vp, vp]),
    "crl_league_reset": (i32, [vp, vp]),
    "crl_league_get_stack": (i32, [vp, vp, vp]),
    "crl_league_set_stack": (i32, [vp, vp, vp]),
    "crl_ledger_create": (i32, [i32, i64, i64, u64, i32, P(vp)]),
    "crl_ledger_destroy": (None, [vp]),
    "crl_ledger_seed": (i32, [vp, u64, vp]),
    "crl_ledger_reset": (i32, [vp, vp]),
    "crl_ledger_set_agents": (i32, [vp, i32, vp]),
    "crl_ledger_set_weights": (i32, [vp, vp, i32, vp]),
    "crl_ledger_get_weights": (i32, [vp, vp, vp]),
    "crl_ledger_pfsp_weights": (i32, [vp, vp, i32, i32, u32, vp]),
    "crl_ledger_get_counters": (i32, [vp, vp, vp, vp]),
    "crl_ledger_set_counters": (i32, [vp, vp, vp, vp]),
    "crl_ledger_get_env_state": (i32, [vp, vp, vp, vp, vp]),
    "crl_ledger_set_env_state": (i32, [vp, vp, vp, vp, vp]),
    "crl_ledger_step": (i32, [vp, vp, vp, i64, vp, i32, vp, vp]),
    "crl_arena_create": (i32, [i32, i64, i64, u64, i32, P(vp)]),
    "crl_arena_destroy": (None, [vp]),
    "crl_arena_seed": (i32, [vp, u64, vp]),
    "crl_arena_reset": (i32, [vp, vp]),
    "crl_arena_set_agents": (i32, [vp, i32, vp]),
    "crl_arena_set_weights": (i32, [vp, vp, i32, vp]),
    "crl_arena_get_weights": (i32, [vp, vp, vp]),
    "crl_arena_balance_weights": (i32, [vp, vp, i32, u32, vp]),
    "crl_arena_get_counters": (i32, [vp, vp, vp, vp]),
    "crl_arena_set_counters": (i32, [vp, vp, vp, vp]),
    "crl_arena_get_env_state": (i32, [vp, vp, vp, vp, vp]),
    "crl_arena_set_env_state": (i32, [vp, vp, vp, vp, vp]),
    "crl_arena_draw": (i32, [vp, vp, vp, vp]),
    "crl_arena_step": (i32, [vp, vp, vp, i64, vp, i32, vp, vp]),
    "crl_rollout_create": (i32, [i32, i64, i64, P(vp)]),
    "crl_rollout_destroy": (None, [vp]),
    "crl_rollout_begin": (i32, [vp, vp, vp]),
    "crl_rollout_record": (i32, [vp, i64, vp, i64, vp, vp, i64, vp, vp, vp]),
    "crl_rollout_outcome": (i32, [vp, i64, vp, i64, vp, vp]),
    "crl_rollout_finish": (i32, [vp, vp, f64, f64, i32, vp]),
    "crl_rollout_gather": (i32, [vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, vp]),
    "crl_rollout_stats": (i32, [vp, P(f64)]),
    "crl_ppo_create": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, P(vp)]),
    "crl_ppo_destroy": (None, [vp]),
    "crl_ppo_set_weights": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_ppo_get_weights": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_ppo_weights_dev": (i32, [vp, P(vp)]),
    "crl_ppo_grad": (i32, [vp, vp, vp, i64, vp, vp]),
    "crl_ppo_get_grad": (i32, [vp, P(vp), vp]),
    "crl_ppo_step": (i32, [vp, vp, vp]),
    "crl_ppo_stats": (i32, [vp, P(f64)]),
    "crl_policy_load_weights_dev": (i32, [vp, vp, vp]),
    "crl_pool_load_light_dev": (i32, [vp, i32, vp, vp]),
    "crl_ppo_create_full": (i32, [i32, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, P(vp)]),
    "crl_ppo_set_weights_full": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_ppo_get_weights_full": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_policy_load_full_dev": (i32, [vp, vp, vp]),
    "crl_pool_load_full_dev": (i32, [vp, i32, vp, vp]),
    "crl_policy_get_blob": (i32, [vp, vp, i64, P(i32), vp]),
    "crl_policy_get_sampling": (i32, [vp, P(f32), P(f32), P(u64), P(i64), P(u32)]),
    "crl_policy_resume_sampling": (i32, [vp, f32, f32, u64, i64, u32]),
    "crl_pool_get_blob": (i32, [vp, i32, vp, i64, vp]),
    "crl_pool_get_counters": (i32, [vp, P(u64), P(i64), P(u32), vp, vp]),
    "crl_pool_set_counters": (i32, [vp, u32, vp, vp]),
    "crl_rollout_get_info": (i32, [vp, P(i32)]),
    "crl_rollout_get_state": (i32, [vp, i64, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_rollout_set_state": (i32, [vp, P(i32), i64, i64, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_ppo_get_state": (i32, [vp, vp, vp, vp, i64, P(i64), P(i64), vp]),
    "crl_ppo_set_state": (i32, [vp, vp, vp, vp, i64, i64, vp]),
    "crl_car_driver_create": (i32, [vp, u64, P(vp)]),
    "crl_car_driver_destroy": (None, [vp]),
    "crl_car_driver_set_style": (i32, [vp, i32, i32, f32, i32, f32, f32]),
    "crl_car_driver_get_style": (i32, [vp, i32, P(i32), P(f32), P(i32), P(f32), P(f32)]),
    "crl_car_driver_set_assignment": (i32, [vp, vp, vp]),
    "crl_car_driver_get_assignment": (i32, [vp, vp, vp]),
    "crl_car_driver_act": (i32, [vp, vp, vp]),
    "crl_car_driver_get_counters": (i32, [vp, P(u64), P(i64)]),
    "crl_car_driver_set_counters": (i32, [vp, u64, i64]),
    "crl_car_policy_create": (i32, [vp, u64, P(vp)]),
    "crl_car_policy_destroy": (None, [vp]),
    "crl_car_policy_set_weights": (i32, [vp, i32, vp, i32, vp]),
    "crl_car_policy_get_weights": (i32, [vp, i32, vp, P(i32), vp]),
    "crl_car_policy_set_sampling": (i32, [vp, i32, i32]),
    "crl_car_policy_set_assignment": (i32, [vp, vp, vp]),
    "crl_car_policy_get_assignment": (i32, [vp, vp, vp]),
    "crl_car_policy_act": (i32, [vp, vp, vp, vp, vp, vp, vp]),
    "crl_car_policy_observe": (i32, [vp, vp, vp]),
    "crl_car_policy_get_counters": (i32, [vp, P(u64), P(i64)]),
    "crl_car_policy_set_counters": (i32, [vp, u64, i64]),
    "crl_rule_labels": (i32, [vp, i32, vp, i64, vp]),
    "crl_ppo_grad_teacher": (i32, [vp, vp, vp, i64, vp, vp, vp]),
    "crl_ppo_teacher_stats": (i32, [vp, P(f64)]),
    "crl_car_rollout_create": (i32, [vp, i64, i32, P(vp)]),
    "crl_car_rollout_destroy": (None, [vp]),
    "crl_car_rollout_begin": (i32, [vp]),
    "crl_car_rollout_record": (i32, [vp, i64, vp, i32, vp, vp, vp, vp, vp]),
    "crl_car_rollout_outcome": (i32, [vp, i64, vp, vp, vp]),
    "crl_car_rollout_finish": (i32, [vp, vp, f64, f64, i32, vp]),
    "crl_car_rollout_gather": (i32, [vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    "crl_car_rollout_stats": (i32, [vp, P(f64)]),
    "crl_car_rollout_get_info": (i32, [vp, P(i32)]),
    "crl_car_rollout_get_state": (i32, [vp, i64, vp, vp, vp]),
    "crl_car_rollout_set_state": (i32, [vp, P(i32), i64, vp, vp, vp]),
    "crl_car_ppo_create": (i32, [i32, vp, P(vp)]),
    "crl_car_ppo_destroy": (None, [vp]),
    "crl_car_ppo_set_weights": (i32, [vp, vp]),
    "crl_car_ppo_get_weights": (i32, [vp, vp]),
    "crl_car_ppo_weights_dev": (i32, [vp, P(vp)]),
    "crl_car_ppo_grad": (i32, [vp, vp, vp, i64, vp, vp]),
    "crl_car_ppo_grad_teacher": (i32, [vp, vp, vp, i64, vp, vp, vp]),
    "crl_car_ppo_teacher_stats": (i32, [vp, P(f64)]),
    "crl_car_ppo_get_grad": (i32, [vp, P(vp), vp]),
    "crl_car_ppo_step": (i32, [vp, vp, vp]),
    "crl_car_ppo_stats": (i32, [vp, P(f64)]),
    "crl_car_ppo_get_state": (i32, [vp, vp, vp, vp, P(i64), vp]),
    "crl_car_ppo_set_state": (i32, [vp, vp, vp, vp, i64, vp]),
    "crl_car_league_create": (i32, [vp, vp, vp, u64, P(vp)]),
    "crl_car_league_destroy": (None, [vp]),
    "crl_car_league_add_agent": (i32, [vp, i32, i32, P(i32), vp]),
    "crl_car_league_get_pool": (i32, [vp, P(i32), vp, vp]),
    "crl_car_league_draw_all": (i32, [vp, vp]),
    "crl_car_league_seed": (i32, [vp, u64, vp]),
    "crl_car_league_reset": (i32, [vp, vp]),
    "crl_car_league_reset_agent": (i32, [vp, i32, vp]),
    "crl_car_league_set_weights": (i32, [vp, vp, i32, vp]),
    "crl_car_league_get_weights": (i32, [vp, vp, vp]),
    "crl_car_league_pfsp_weights": (i32, [vp, vp, i32, i32, u32, vp]),
    "crl_car_league_get_counters": (i32, [vp, vp, vp]),
    "crl_car_league_set_counters": (i32, [vp, vp, vp]),
    "crl_car_league_get_env_state": (i32, [vp, vp, vp, vp, vp, vp]),
    "crl_car_league_set_env_state": (i32, [vp, vp, vp, vp, vp, vp]),
    "crl_car_league_get_assignment": (i32, [vp, vp, vp]),
    "crl_car_league_step": (i32, [vp, vp, vp, i32, vp]),
}
SYMBOLS = list(SIGNATURES)


class CrlError(RuntimeError):
    pass


class CrlActionError(CrlError, AssertionError):
    """An action outside the action space reached the step kernel (the reference's
    ``assert self.action_space.contains(action)``, pong/base_pong_env.py:42)."""


_lib = None


def load():
    """Load libcrl_hip.so or raise -- the product path never silently degrades."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m competitive_rl_amd.build` "
            "(hipcc, gfx950).  competitive_rl_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = f"crl error {rc}: {load().crl_last_error().decode()}"
        raise (CrlActionError if rc == CRL_EACTION else CrlError)(msg)


def load_score_atlas():
    a = np.load(os.path.join(PKG, "assets", "pong_score_atlas.npz"))["atlas"]
    a = np.ascontiguousarray(a, dtype=np.uint8)
    assert a.size == ATLAS_BYTES
    return a


def load_car_text():
    b = np.load(os.path.join(PKG, "assets", "car_reward_text.npz"))["bits"]
    b = np.ascontiguousarray(b, dtype=np.uint32)
    assert b.shape == (3001, 10)
    return b
