"""ctypes binding of libfo_hip.so (C ABI: include/fo_hip.h).

The HIP library is the product path.  There is NO CPU fallback: if the library is missing, fails to load, or no
GPU is visible, every entry point raises.  PyTorch is used only as the owner of device memory and streams.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FO_HIP_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libfo_hip.so")  # env: tuning builds

FO_OK, FO_E_ARG, FO_E_UNSUPPORTED_COV, FO_E_HIP, FO_E_NOMEM, FO_E_STATE = 0, -1, -2, -3, -4, -5
NPF, NPI, NL, NC = 12, 4, 5, 16
LISTS_F64, LISTS_F32, LISTS_F32_EXACT = 0, 1, 2
LIST_FORMAT = {"f64": LISTS_F64, "f32": LISTS_F32, "f32x": LISTS_F32_EXACT}   # f32x: float64 arithmetic, float32 store

PF = {"dce": 0, "ttc": 1, "ttce": 2, "max_ego_risk": 3, "max_obst_risk": 4, "max_obst_harm_with_cp": 5,
      "max_ego_harm": 6, "max_obst_harm": 7, "max_collision_probability": 8, "be_decel": 9, "be_btn": 10}
PI = {"time_dce": 0, "max_obst_risk_index": 1, "cp_argmax": 2, "hr_valid": 3}
LST = {"cp": 0, "ego_harm": 1, "obst_harm": 2, "ego_risk": 3, "obst_risk": 4}
COST = {"wttc": 0, "min_dce": 1, "max_ego_risk_all": 2, "max_obst_risk_all": 3, "max_ego_harm_all": 4,
        "max_obst_harm_all": 5, "max_collision_probability_all": 6, "max_obst_harm_with_cp_all": 7, "min_ttce": 8,
        "argmin_dce": 9, "argmin_ttc": 10, "argmax_risk": 11, "safe": 12, "max_btn": 13}
METRIC_BITS = {"dce": 1, "cp": 2, "ttc": 4, "ttce": 8, "wttc": 16, "be": 32, "hr": 64}
TYPE_CODES = {"car": 0, "truck": 1, "bus": 2, "bicycle": 3, "pedestrian": 4, "priorityvehicle": 5,
              "parkedvehicle": 6, "train": 7, "motorcycle": 8, "taxi": 9, "unknown": 10}

LEN_REFUSED = -2**31     # FO_LEN_REFUSED (INT32_MIN): the length in the first rule slot of a refused rule list (include/fo_hip.h)


def _header_constant(header, name):
    """an integer ``constexpr int NAME = value;`` of a csrc header the library is built from: the one place the number is
    written down (the package carries its sources next to the library, __graft_entry__.build compiles them)"""
    import re
    with open(os.path.join(os.path.dirname(_HERE), "csrc", header)) as f:
        m = re.search(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, f.read())
    if not m:
        raise ImportError(f"{header}: no integer constant {name}")
    return int(m.group(1))


RULE_MAX_SAMPLES = _header_constant("fo_rule_plan.hpp", "RL_MAXSAMP")   # samples of a rule line (one every cell / 8) the device holds

# every symbol include/fo_hip.h declares (tests check the library exports all of them)
EXPORTS = [
    "fo_abi_version", "fo_build_id", "fo_create", "fo_destroy", "fo_last_error",
    "fo_sweep_configure", "fo_sweep_reserve", "fo_sweep_set_list_format", "fo_sweep_set_agents", "fo_sweep_run", "fo_sweep_check",
    "fo_sweep_last_launch", "fo_sweep_timing", "fo_sweep_timing_read", "fo_sweep_timing_read_each",
    "fo_scene_set_map", "fo_scene_share_map", "fo_scene_set_edge_lines", "fo_scene_set_routes", "fo_scene_map_info", "fo_scene_copy_raster", "fo_scene_fan", "fo_scene_visibility", "fo_scene_future_visibility", "fo_scene_spawn",
    "fo_scene_candidate_count", "fo_scene_set_topology", "fo_scene_spawn_rules", "fo_step_run", "fo_step_mirror_wait",
    "fo_scene_set_centerlines", "fo_scene_spawn_rule_agents", "fo_sweep_autotune", "fo_scene_set_shadow_length",
    "fo_scene_set_occlusion_memory", "fo_scene_future_visibility_ex", "fo_scene_hidden_reach",
    "fo_scene_hidden_reach_road", "fo_scene_hidden_clearance", "fo_scene_set_occlusion_memory_road",
    "fo_scene_set_lane_moves", "fo_scene_hidden_reach_flow", "fo_scene_hidden_clearance_flow",
    "fo_scene_set_occlusion_memory_vehicles", "fo_scene_hidden_witness", "fo_scene_hidden_brake",
    "fo_scene_hidden_brake_classes", "fo_scene_hidden_brake_users", "fo_scene_hidden_brake_ladder",
    "fo_scene_hidden_brake_ladder_users", "fo_scene_hidden_poses", "fo_scene_hidden_brake_verdict",
    "fo_scene_hidden_brake_ladder_verdict", "fo_scene_hidden_brake_impact", "fo_hidden_impact_row",
    "fo_scene_hidden_brake_impact_lanes", "fo_scene_hidden_brake_harm_ladder", "fo_scene_hidden_brake_harm_ladder_lanes",
]


class Vehicle(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("length", "width", "wb_rear_axle", "mass", "a_max")]


class HarmCoeff(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("lr4s_const", "lr4s_speed", "lr4s_side", "lr4s_rear", "lr1s_const",
                                          "lr1s_speed", "ped_const", "ped_speed")]


class Thresholds(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("harm", "risk", "be", "cp", "ttc", "dce")]


class SpawnRuleParams(C.Structure):       # fo_spawn_rule_params_t
    _fields_ = ([(n, C.c_double) for n in ("ego_x", "ego_y", "ego_yaw", "ego_s", "ego_d", "s_threshold", "ped_width", "ped_length")] +
                [(n, C.c_int32) for n in ("intention", "win_i0", "win_i1", "behind_static", "behind_turn", "behind_dynamic",
                                          "max_static", "max_dynamic", "n_dynamic_plus1", "frame")])


class RuleAgentTypes(C.Structure):       # fo_rule_agent_types_t: index 0 Car, 1 Bicycle, 2 Pedestrian
    _fields_ = [(n, C.c_double * 3) for n in ("speed", "raw_l", "raw_w", "infl_l", "infl_w")]


OCCLUSION_MEMORY_MAX_HALO = 32     # FO_OCCLUSION_MEMORY_MAX_HALO: the largest reach (cells) the memory kernel stages


class OcclusionMemory(C.Structure):     # fo_occlusion_memory_t
    _fields_ = [("r2", C.c_int32), ("reset", C.c_int32), ("prev_ix0", C.c_int32), ("prev_iy0", C.c_int32),
                ("prev_nx", C.c_int32), ("prev_ny", C.c_int32), ("d_prev", C.c_void_p), ("d_cur", C.c_void_p),
                ("prev_bytes", C.c_int64), ("cur_bytes", C.c_int64)]


FUTURE_VISIBILITY_MAX_CELLS = 114688    # FO_FUTURE_VISIBILITY_MAX_CELLS: the largest window the first-seen outputs take


class FutureVisibility(C.Structure):    # fo_future_visibility_t
    _fields_ = [("M", C.c_int32), ("T", C.c_int32), ("t_stride", C.c_int32), ("n_rays", C.c_int32),
                ("d_x", C.c_void_p), ("d_y", C.c_void_p), ("d_dirs", C.c_void_p), ("r", C.c_double), ("fov_deg", C.c_double),
                ("d_heading", C.c_void_p), ("O", C.c_int32), ("n_slices", C.c_int32), ("d_ocorn", C.c_void_p),
                ("d_oflags", C.c_void_p), ("d_occ_idx", C.c_void_p), ("d_n_occ", C.c_void_p), ("win_ix0", C.c_int32),
                ("win_iy0", C.c_int32), ("win_nx", C.c_int32), ("win_ny", C.c_int32), ("d_revealed", C.c_void_p),
                ("d_area", C.c_void_p), ("d_revealed_new", C.c_void_p), ("d_revealed_any", C.c_void_p)]


HIDDEN_REACH_MAX_HALO = 254      # FO_HIDDEN_REACH_MAX_HALO: the longest reach (cells) of the hidden-traffic forecast
HIDDEN_REACH_MAX_HALF_EXTENT = 64   # FO_HIDDEN_REACH_MAX_HALF_EXTENT: the largest half extent of its ego rectangle (cells)
HIDDEN_REACH_MAX_J = 254         # samples of its horizon (arrival steps are bytes, 255 = never)


class HiddenReach(C.Structure):         # fo_hidden_reach_t
    _fields_ = [("M", C.c_int32), ("T", C.c_int32), ("d_x", C.c_void_p), ("d_y", C.c_void_p), ("d_heading", C.c_void_p),
                ("d_len_or_null", C.c_void_p), ("hl", C.c_double), ("hw", C.c_double), ("wb", C.c_double), ("J", C.c_int32),
                ("h_r2", C.POINTER(C.c_int32)), ("d_cls", C.c_void_p), ("d_hidden_or_null", C.c_void_p),
                ("win_ix0", C.c_int32), ("win_iy0", C.c_int32), ("win_nx", C.c_int32), ("win_ny", C.c_int32),
                ("d_arrival", C.c_void_p), ("d_cells", C.c_void_p), ("d_first", C.c_void_p), ("d_slack", C.c_void_p)]


class HiddenReachRoad(C.Structure):     # fo_hidden_reach_road_t
    _fields_ = [("base", HiddenReach), ("d_dist_or_null", C.c_void_p)]


HIDDEN_WITNESS_MAX_STEPS = 276   # FO_HIDDEN_WITNESS_MAX_STEPS: the longest walk at the halo cap


class HiddenWitness(C.Structure):       # fo_hidden_witness_t
    _fields_ = [("base", HiddenReach), ("d_dist", C.c_void_p), ("flow", C.c_int32), ("path_cap", C.c_int32),
                ("d_cell", C.c_void_p), ("d_src", C.c_void_p), ("d_steps", C.c_void_p), ("d_wdist", C.c_void_p),
                ("d_dirs", C.c_void_p)]


class HiddenBrake(C.Structure):         # fo_hidden_brake_t
    _fields_ = [("base", HiddenReach), ("d_v", C.c_void_p), ("d_arc", C.c_void_p), ("a_brake", C.c_double), ("dt", C.c_double),
                ("d_brake_first", C.c_void_p), ("d_stop", C.c_void_p), ("d_commit", C.c_void_p)]


HIDDEN_BRAKE_MAX_CLASSES = 8    # FO_HIDDEN_BRAKE_MAX_CLASSES: classes of hidden road users one fo_scene_hidden_brake_classes call serves
HIDDEN_BRAKE_MAX_TABLE = 896    # FO_HIDDEN_BRAKE_MAX_TABLE: entries C * T of its threshold table (a kernel argument)


class HiddenBrakeClasses(C.Structure):  # fo_hidden_brake_classes_t
    _fields_ = [("M", C.c_int32), ("T", C.c_int32), ("d_x", C.c_void_p), ("d_y", C.c_void_p), ("d_heading", C.c_void_p),
                ("d_len_or_null", C.c_void_p), ("hl", C.c_double), ("hw", C.c_double), ("wb", C.c_double),
                ("win_ix0", C.c_int32), ("win_iy0", C.c_int32), ("win_nx", C.c_int32), ("win_ny", C.c_int32),
                ("r2_cap", C.c_int32), ("C", C.c_int32), ("d_key", C.c_void_p), ("d_qmin", C.c_void_p), ("d_v", C.c_void_p),
                ("d_arc", C.c_void_p), ("a_brake", C.c_double), ("dt", C.c_double), ("h_thr", C.POINTER(C.c_int32)),
                ("d_brake_first", C.c_void_p), ("d_stop", C.c_void_p), ("d_commit", C.c_void_p), ("d_first", C.c_void_p)]


HIDDEN_BRAKE_MAX_MAPS = 3       # FO_HIDDEN_BRAKE_MAX_MAPS: key maps (forecasts) one fo_scene_hidden_brake_users call walks over

# the members the four structures of the users family (brake_users, ladder_users, verdict, ladder_verdict) begin with, up to d_arc
_HIDDEN_USERS_HEAD = [("M", C.c_int32), ("T", C.c_int32), ("d_x", C.c_void_p), ("d_y", C.c_void_p), ("d_heading", C.c_void_p),
                      ("d_len_or_null", C.c_void_p), ("hl", C.c_double), ("hw", C.c_double), ("wb", C.c_double),
                      ("win_ix0", C.c_int32), ("win_iy0", C.c_int32), ("win_nx", C.c_int32), ("win_ny", C.c_int32),
                      ("K", C.c_int32), ("C", C.c_int32), ("d_key", C.c_void_p * HIDDEN_BRAKE_MAX_MAPS),
                      ("d_qmin", C.c_void_p * HIDDEN_BRAKE_MAX_MAPS), ("r2_cap", C.c_int32 * HIDDEN_BRAKE_MAX_MAPS),
                      ("map_of", C.c_int32 * HIDDEN_BRAKE_MAX_CLASSES), ("d_v", C.c_void_p), ("d_arc", C.c_void_p)]


class HiddenBrakeUsers(C.Structure):    # fo_hidden_brake_users_t
    _fields_ = _HIDDEN_USERS_HEAD + [
        ("a_brake", C.c_double), ("dt", C.c_double), ("h_thr", C.POINTER(C.c_int32)),
        ("d_brake_first", C.c_void_p), ("d_stop", C.c_void_p), ("d_commit", C.c_void_p), ("d_first", C.c_void_p)]


HIDDEN_BRAKE_MAX_LEVELS = 64    # FO_HIDDEN_BRAKE_MAX_LEVELS: decelerations one fo_scene_hidden_brake_ladder call evaluates


class HiddenBrakeLadder(C.Structure):   # fo_hidden_brake_ladder_t
    _fields_ = [("base", HiddenReach), ("d_v", C.c_void_p), ("d_arc", C.c_void_p), ("h_levels", C.POINTER(C.c_double)),
                ("K", C.c_int32), ("B", C.c_int32), ("dt", C.c_double), ("d_brake_first", C.c_void_p), ("d_stop", C.c_void_p),
                ("d_required", C.c_void_p), ("d_last_unclear", C.c_void_p), ("d_commit", C.c_void_p)]


# FO_HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES: 4 bytes per threshold (C * T) and 8 per level of one fo_scene_hidden_brake_ladder_users call
HIDDEN_BRAKE_LADDER_USERS_MAX_ARG_BYTES = 3584


class HiddenBrakeLadderUsers(C.Structure):      # fo_hidden_brake_ladder_users_t
    _fields_ = _HIDDEN_USERS_HEAD + [
        ("h_levels", C.POINTER(C.c_double)), ("L", C.c_int32), ("B", C.c_int32), ("dt", C.c_double),
        ("h_thr", C.POINTER(C.c_int32)), ("d_required", C.c_void_p), ("d_last_unclear", C.c_void_p), ("d_commit", C.c_void_p),
        ("d_first", C.c_void_p), ("d_required_all", C.c_void_p), ("d_last_unclear_all", C.c_void_p), ("d_blocking", C.c_void_p),
        ("d_brake_first_or_null", C.c_void_p), ("d_stop_or_null", C.c_void_p)]


class HiddenPoses(C.Structure):         # fo_hidden_poses_t
    _fields_ = [("M", C.c_int32), ("T", C.c_int32), ("d_x", C.c_void_p), ("d_y", C.c_void_p), ("d_theta", C.c_void_p),
                ("d_v", C.c_void_p), ("d_len_or_null", C.c_void_p), ("d_heading", C.c_void_p), ("d_arc", C.c_void_p),
                ("d_finite", C.c_void_p)]


HIDDEN_VERDICT_NOT_FINITE = -2  # FO_HIDDEN_VERDICT_NOT_FINITE: user[m] of a candidate with a non-finite pose


class HiddenBrakeVerdict(C.Structure):  # fo_hidden_brake_verdict_t
    _fields_ = _HIDDEN_USERS_HEAD + [
        ("a_brake", C.c_double), ("dt", C.c_double), ("h_thr", C.POINTER(C.c_int32)), ("B", C.c_int32),
        ("commit_min", C.c_int32), ("d_finite_or_null", C.c_void_p), ("d_cost_or_null", C.c_void_p),
        ("d_safe_or_null", C.c_void_p), ("d_fail_safe", C.c_void_p), ("d_user", C.c_void_p), ("d_commit", C.c_void_p),
        ("d_first", C.c_void_p)]


class HiddenBrakeLadderVerdict(C.Structure):    # fo_hidden_brake_ladder_verdict_t
    _fields_ = _HIDDEN_USERS_HEAD + [
        ("h_levels", C.POINTER(C.c_double)), ("L", C.c_int32), ("B", C.c_int32), ("dt", C.c_double),
        ("h_thr", C.POINTER(C.c_int32)), ("a_limit", C.c_double), ("d_finite_or_null", C.c_void_p),
        ("d_cost_or_null", C.c_void_p), ("d_safe_or_null", C.c_void_p), ("d_need", C.c_void_p), ("d_at", C.c_void_p),
        ("d_blocking", C.c_void_p), ("d_user", C.c_void_p), ("d_decel", C.c_void_p), ("d_need_of", C.c_void_p),
        ("d_first", C.c_void_p)]


class HiddenBrakeImpact(C.Structure):   # fo_hidden_brake_impact_t
    _fields_ = _HIDDEN_USERS_HEAD + [
        ("a_brake", C.c_double), ("dt", C.c_double), ("h_thr", C.POINTER(C.c_int32)), ("B", C.c_int32),
        ("d_speed_of", C.c_void_p), ("d_harm_rows", C.c_void_p), ("harm_limit", C.c_double), ("d_finite_or_null", C.c_void_p),
        ("d_cost_or_null", C.c_void_p), ("d_safe_or_null", C.c_void_p), ("d_harm", C.c_void_p), ("d_user", C.c_void_p),
        ("d_speed", C.c_void_p), ("d_at", C.c_void_p), ("d_commit", C.c_void_p), ("d_first", C.c_void_p)]


class HiddenBrakeImpactLanes(C.Structure):      # fo_hidden_brake_impact_lanes_t
    _fields_ = [(("d_closing", t) if n == "d_speed" else (n, t)) for n, t in HiddenBrakeImpact._fields_] + [
        ("dir_mask", C.c_uint32), ("cos_h", C.c_double), ("sin_h", C.c_double), ("d_cosine", C.c_void_p)]


class HiddenBrakeHarmLadder(C.Structure):       # fo_hidden_brake_harm_ladder_t
    _fields_ = HiddenBrakeLadderVerdict._fields_ + [
        ("d_speed_of", C.c_void_p), ("d_harm_rows", C.c_void_p), ("harm_limit", C.c_double), ("d_harm_at", C.c_void_p),
        ("d_user_at", C.c_void_p)]


class HiddenBrakeHarmLadderLanes(C.Structure):  # fo_hidden_brake_harm_ladder_lanes_t
    _fields_ = HiddenBrakeHarmLadder._fields_ + [("dir_mask", C.c_uint32), ("cos_h", C.c_double), ("sin_h", C.c_double)]


HIDDEN_CLEARANCE_NONE = 2 ** 31 - 1  # FO_HIDDEN_CLEARANCE_NONE: the key of a cell (the clearance of a pose) nothing within the cap reaches
HIDDEN_CLEARANCE_METRIC = {"euclid": 0, "road": 1}   # FO_HIDDEN_CLEARANCE_EUCLID / _ROAD


class HiddenClearance(C.Structure):     # fo_hidden_clearance_t
    _fields_ = [("M", C.c_int32), ("T", C.c_int32), ("d_x", C.c_void_p), ("d_y", C.c_void_p), ("d_heading", C.c_void_p),
                ("d_len_or_null", C.c_void_p), ("hl", C.c_double), ("hw", C.c_double), ("wb", C.c_double),
                ("r2_cap", C.c_int32), ("metric", C.c_int32), ("d_cls", C.c_void_p), ("d_hidden_or_null", C.c_void_p),
                ("win_ix0", C.c_int32), ("win_iy0", C.c_int32), ("win_nx", C.c_int32), ("win_ny", C.c_int32),
                ("d_key", C.c_void_p), ("d_qmin", C.c_void_p), ("d_dist_or_null", C.c_void_p)]


SPAWN_CELLS, SPAWN_RULES, SPAWN_BOTH = 0, 1, 2
SPAWN_MODE = {"cells": SPAWN_CELLS, "rules": SPAWN_RULES, "both": SPAWN_BOTH}


class Step(C.Structure):       # fo_step_t (include/fo_hip.h): the arguments of one planning step's five stage calls
    _fields_ = [("n_rays", C.c_int32), ("polygon_footprint", C.c_int32), ("ego_yaw", C.c_double), ("fov_deg", C.c_double),
                ("r", C.c_double), ("d_dirs", C.c_void_p), ("d_rmax", C.c_void_p), ("d_half", C.c_void_p),
                ("ego_x", C.c_double), ("ego_y", C.c_double), ("head_x", C.c_double), ("head_y", C.c_double),
                ("full_circle", C.c_int32), ("exact_cells", C.c_int32), ("O", C.c_int32), ("d_edge_skip", C.c_void_p),
                ("d_ocorn", C.c_void_p), ("d_ocen", C.c_void_p), ("d_oflags", C.c_void_p),
                ("win_ix0", C.c_int32), ("win_iy0", C.c_int32), ("win_nx", C.c_int32), ("win_ny", C.c_int32),
                ("d_range", C.c_void_p), ("d_hit_id", C.c_void_p), ("d_ring", C.c_void_p), ("d_obst_vis", C.c_void_p),
                ("d_cls", C.c_void_p), ("d_occ_idx", C.c_void_p), ("d_n_occ", C.c_void_p),
                ("min_ahead", C.c_double), ("max_dist", C.c_double), ("all_occluded", C.c_int32), ("max_agents", C.c_int32),
                ("routes", C.c_int32), ("n_path", C.c_int32), ("T_agents", C.c_int32), ("type4", C.c_int32 * 4),
                ("speed4", C.c_double * 4), ("raw_l4", C.c_double * 4), ("raw_w4", C.c_double * 4),
                ("infl_l4", C.c_double * 4), ("infl_w4", C.c_double * 4), ("d_path", C.c_void_p), ("dt", C.c_double),
                ("var0", C.c_double), ("var_factor", C.c_double), ("d_cell", C.c_void_p), ("d_pos0", C.c_void_p),
                ("d_yaw0", C.c_void_p), ("d_n", C.c_void_p), ("d_pos", C.c_void_p), ("d_yaw", C.c_void_p), ("d_v", C.c_void_p),
                ("d_cov", C.c_void_p), ("d_shape", C.c_void_p), ("d_raw_dims", C.c_void_p), ("d_type", C.c_void_p),
                ("d_len", C.c_void_p), ("M", C.c_int32), ("T", C.c_int32), ("d_x", C.c_void_p), ("d_y", C.c_void_p),
                ("d_theta", C.c_void_p), ("d_vel", C.c_void_p), ("d_acc", C.c_void_p), ("d_cost", C.c_void_p),
                ("d_safe", C.c_void_p), ("d_pair_f", C.c_void_p), ("d_pair_i", C.c_void_p), ("d_lists", C.c_void_p),
                ("list_format", C.c_int32), ("spawn_mode", C.c_int32), ("n_path6", C.c_int32), ("max_rule_points", C.c_int32),
                ("d_path6", C.c_void_p), ("d_oyaw", C.c_void_p), ("d_odims", C.c_void_p), ("rule", SpawnRuleParams),
                ("rule_types", RuleAgentTypes), ("d_rule_points", C.c_void_p), ("d_n_rule_points", C.c_void_p),
                # ABI 12: the step's own host transfers (obstacle rows in, hit ids + visibility flags out)
                ("h_obstacles", C.c_void_p), ("d_obstacles", C.c_void_p), ("obstacles_bytes", C.c_int64),
                ("h_mirror", C.c_void_p), ("d_mirror", C.c_void_p), ("mirror_bytes", C.c_int64)]


class NativeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libfo_hip error {code}: {msg}")
        self.code = code


_lib = None


def load():
    """Load libfo_hip.so or raise (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not found: build it with `python __graft_entry__.py build` "
                          "(hipcc --offload-arch=gfx950); there is no CPU fallback")
    # PyTorch ships its own libamdhip64; the process must end up with ONE HIP runtime, the one torch allocates with.
    # Loaded after torch, libfo_hip.so binds to that copy (same soname); loaded first it would pull in /opt/rocm's, torch
    # would then bring a second runtime, and fo_create would fail on a device the other runtime owns.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    vp, dp, ip = C.c_void_p, C.c_void_p, C.c_void_p
    lib.fo_abi_version.restype = C.c_int
    lib.fo_build_id.restype = C.c_char_p
    lib.fo_create.argtypes = [C.POINTER(vp), C.c_int]
    lib.fo_destroy.argtypes = [vp]
    lib.fo_destroy.restype = None
    lib.fo_last_error.argtypes = [vp]
    lib.fo_last_error.restype = C.c_char_p
    lib.fo_sweep_configure.argtypes = [vp, C.POINTER(Vehicle), C.POINTER(HarmCoeff), C.POINTER(Thresholds),
                                       C.c_uint32, C.c_double]
    lib.fo_sweep_reserve.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int]
    lib.fo_sweep_set_list_format.argtypes = [vp, C.c_int]
    lib.fo_sweep_set_agents.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, ip, ip, vp]
    lib.fo_sweep_run.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, ip, dp, vp]
    lib.fo_sweep_check.argtypes = [vp, vp]
    lib.fo_sweep_autotune.argtypes = [vp, C.c_int, C.c_int, dp, dp, dp, dp, dp, dp, dp, dp, ip, dp, C.c_int, C.POINTER(C.c_int),
                                      C.POINTER(C.c_double), vp]
    lib.fo_sweep_timing.argtypes = [vp, C.c_int]
    lib.fo_sweep_timing_read.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]
    lib.fo_sweep_timing_read_each.argtypes = [vp, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int)]
    lib.fo_sweep_last_launch.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    D = C.c_double
    lib.fo_scene_set_map.argtypes = [vp, C.c_int, ip, dp, C.c_int, dp, D, D, dp, dp, ip]
    lib.fo_scene_share_map.argtypes = [vp, vp]
    lib.fo_scene_set_routes.argtypes = [vp, C.c_int, C.c_int, ip, ip, C.c_int, dp, dp, ip]
    lib.fo_scene_map_info.argtypes = [vp] + [C.POINTER(D)] * 3 + [C.POINTER(C.c_int)] * 3
    lib.fo_scene_copy_raster.argtypes = [vp, vp]
    lib.fo_scene_set_edge_lines.argtypes = [vp, C.c_int, ip]
    lib.fo_scene_fan.argtypes = [vp, C.c_int, D, D, D, C.c_int, dp, dp, dp, vp]
    lib.fo_scene_visibility.argtypes = ([vp, D, D, D, D, D, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, C.c_int, dp, dp, dp]
                                        + [C.c_int] * 4 + [dp] * 7 + [vp])
    lib.fo_scene_future_visibility.argtypes = ([vp, C.c_int, C.c_int, dp, dp, C.c_int, C.c_int, dp, D, C.c_int, dp, dp, ip, ip]
                                               + [C.c_int] * 3 + [ip, dp, vp])
    lib.fo_scene_future_visibility_ex.argtypes = [vp, C.POINTER(FutureVisibility), vp]
    lib.fo_scene_hidden_reach.argtypes = [vp, C.POINTER(HiddenReach), vp]
    lib.fo_scene_hidden_reach_road.argtypes = [vp, C.POINTER(HiddenReachRoad), vp]
    lib.fo_scene_hidden_clearance.argtypes = [vp, C.POINTER(HiddenClearance), vp]
    lib.fo_scene_set_lane_moves.argtypes = [vp, vp]
    lib.fo_scene_hidden_reach_flow.argtypes = [vp, C.POINTER(HiddenReachRoad), vp]
    lib.fo_scene_hidden_clearance_flow.argtypes = [vp, C.POINTER(HiddenClearance), vp]
    lib.fo_scene_hidden_witness.argtypes = [vp, C.POINTER(HiddenWitness), vp]
    lib.fo_scene_hidden_brake.argtypes = [vp, C.POINTER(HiddenBrake), vp]
    lib.fo_scene_hidden_brake_classes.argtypes = [vp, C.POINTER(HiddenBrakeClasses), vp]
    lib.fo_scene_hidden_brake_users.argtypes = [vp, C.POINTER(HiddenBrakeUsers), vp]
    lib.fo_scene_hidden_brake_ladder.argtypes = [vp, C.POINTER(HiddenBrakeLadder), vp]
    lib.fo_scene_hidden_brake_ladder_users.argtypes = [vp, C.POINTER(HiddenBrakeLadderUsers), vp]
    lib.fo_scene_hidden_poses.argtypes = [vp, C.POINTER(HiddenPoses), vp]
    lib.fo_scene_hidden_brake_verdict.argtypes = [vp, C.POINTER(HiddenBrakeVerdict), vp]
    lib.fo_scene_hidden_brake_ladder_verdict.argtypes = [vp, C.POINTER(HiddenBrakeLadderVerdict), vp]
    lib.fo_scene_hidden_brake_impact.argtypes = [vp, C.POINTER(HiddenBrakeImpact), vp]
    lib.fo_scene_hidden_brake_impact_lanes.argtypes = [vp, C.POINTER(HiddenBrakeImpactLanes), vp]
    lib.fo_scene_hidden_brake_harm_ladder.argtypes = [vp, C.POINTER(HiddenBrakeHarmLadder), vp]
    lib.fo_scene_hidden_brake_harm_ladder_lanes.argtypes = [vp, C.POINTER(HiddenBrakeHarmLadderLanes), vp]
    lib.fo_hidden_impact_row.argtypes = [C.c_int, C.c_double, C.c_double, C.POINTER(HarmCoeff), C.POINTER(C.c_double)]
    lib.fo_scene_spawn.argtypes = ([vp, dp] + [C.c_int] * 4 + [D] * 6 + [C.c_int] * 3 + [ip] + [dp] * 5 + [C.c_int, dp, C.c_int]
                                   + [D] * 3 + [dp] * 12 + [vp])
    lib.fo_scene_candidate_count.argtypes = [vp, ip, vp]
    lib.fo_step_run.argtypes = [vp, C.POINTER(Step), vp]
    lib.fo_step_mirror_wait.argtypes = [vp]
    lib.fo_scene_set_topology.argtypes = [vp, C.c_int, dp, ip, ip, C.c_int, ip, ip, dp]
    lib.fo_scene_spawn_rules.argtypes = ([vp, dp] + [C.c_int] * 5 + [dp, C.c_int] + [dp] * 6 + [C.POINTER(SpawnRuleParams), C.c_int,
                                                                                          dp, ip, vp])
    lib.fo_scene_set_centerlines.argtypes = [vp, C.c_int, ip, dp]
    lib.fo_scene_set_shadow_length.argtypes = [vp, C.c_double]
    lib.fo_scene_set_occlusion_memory.argtypes = [vp, C.POINTER(OcclusionMemory)]
    lib.fo_scene_set_occlusion_memory_road.argtypes = [vp, C.POINTER(OcclusionMemory)]
    lib.fo_scene_set_occlusion_memory_vehicles.argtypes = [vp, C.POINTER(OcclusionMemory)]
    lib.fo_scene_spawn_rule_agents.argtypes = ([vp, C.c_int, dp, ip, C.c_int, C.POINTER(RuleAgentTypes), C.c_int, dp, C.c_int]
                                               + [D] * 3 + [dp] * 8 + [ip, ip, vp])
    for name in EXPORTS:
        fn = getattr(lib, name)
        if name not in ("fo_destroy", "fo_last_error", "fo_build_id"):
            fn.restype = C.c_int
    _lib = lib
    return lib


_pyhost = False


def pyhost():
    """the CPython helper module ``_fo_pyhost`` (csrc/fo_pyhost.c: packs trajectory OBJECTS into the pinned staging buffer
    with the C API), or None when it has not been built -- the callers then use their numpy statement of the same loop.
    (Host glue between Python objects and host memory, not part of the C ABI and not a compute path.)"""
    global _pyhost
    if _pyhost is False:
        _pyhost = None
        try:
            import importlib.machinery
            import importlib.util
            import sysconfig
            path = os.path.join(os.path.dirname(_HERE), "lib", "_fo_pyhost" + (sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
            if os.path.exists(path) and not os.environ.get("FO_NO_PYHOST"):
                loader = importlib.machinery.ExtensionFileLoader("_fo_pyhost", path)
                spec = importlib.util.spec_from_file_location("_fo_pyhost", path, loader=loader)
                mod = importlib.util.module_from_spec(spec)
                loader.exec_module(mod)
                _pyhost = mod
        except Exception:       # a module built for another interpreter: the numpy path serves
            _pyhost = None
    return _pyhost


def build_id():
    """hash of the sources the loaded library was built from (fo_build_id)"""
    return load().fo_build_id().decode()


def current_stream(device_index=None):
    """raw HIP stream handle of torch's current stream.  ``torch.cuda.current_stream().cuda_stream`` walks several
    Python layers (device lookup, Stream object): ~9 us, five times per planning step; the private getter behind it takes
    a fraction of a microsecond."""
    import torch
    if device_index is None:
        device_index = torch.cuda.current_device()
    try:
        return torch._C._cuda_getCurrentRawStream(device_index)
    except AttributeError:      # other torch build: the public, slower way
        return torch.cuda.current_stream(device_index).cuda_stream


def ptr(t):
    """address of a device tensor as a C argument; None (NULL) for no tensor and for one without elements"""
    return t.data_ptr() if t is not None and t.numel() else None


def on_device(a, dev, dtype="float64"):
    """host array or device tensor -> contiguous tensor of ``dtype`` on ``dev``"""
    import numpy as np
    import torch
    t = a if torch.is_tensor(a) else torch.as_tensor(np.ascontiguousarray(a, dtype=getattr(np, dtype)))
    return t.to(dev, getattr(torch, dtype)).contiguous()


def metric_mask(names):
    m = 0
    for n in names:
        if n not in METRIC_BITS:
            raise ValueError(f"unknown metric '{n}'")
        m |= METRIC_BITS[n]
    return m


def make_thresholds(d=None):
    d = d or {}
    return Thresholds(*[float("nan") if d.get(k) is None else float(d[k])
                        for k in ("harm", "risk", "be", "cp", "ttc", "dce")])


class Context:
    """Owns one fo_ctx (one ego vehicle on one GPU)."""

    def __init__(self, device=0):
        self._lib = load()
        self._h = C.c_void_p()
        rc = self._lib.fo_create(C.byref(self._h), int(device))
        if rc != FO_OK:
            raise NativeError(rc, "fo_create failed (is a gfx950 GPU visible? there is no CPU fallback)")
        self.device = int(device)
        self.list_format = "f64"      # element type of the per-timestep lists the context writes (fo_sweep_set_list_format)

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._lib.fo_destroy(h)
            h.value = None        # (no module globals here: __del__ may run while the interpreter shuts down)

    __del__ = close

    def _check(self, rc):
        if rc != FO_OK:
            raise NativeError(rc, self._lib.fo_last_error(self._h).decode())

    def call(self, name, *args):
        self._check(getattr(self._lib, name)(self._h, *args))

    def timing(self, enable=True, every=1):
        """HIP-event timing of the sweep kernel; every = k > 1 times every k-th launch only"""
        self.call("fo_sweep_timing", (max(int(every), 1) if enable else 0))

    def timing_read(self):
        ms, n = C.c_double(), C.c_int()
        self._check(self._lib.fo_sweep_timing_read(self._h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def timing_read_each(self, cap=1024):
        """durations (ms) of the timed launches, one by one"""
        buf, n = (C.c_double * cap)(), C.c_int()
        self._check(self._lib.fo_sweep_timing_read_each(self._h, buf, cap, C.byref(n)))
        return list(buf[:min(n.value, cap)])

    def last_launch(self):
        g, b, a = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.fo_sweep_last_launch(self._h, C.byref(g), C.byref(b), C.byref(a)))
        return {"grid": g.value, "block": b.value, "agents_per_wave": a.value}
