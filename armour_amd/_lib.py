"""ctypes binding of armour_amd/lib/libarmour_hip.so (the C ABI in include/armour_hip.h).

There is no CPU path: if the shared library is missing or fails to load this module raises, and
`armour_create` fails with ARMOUR_EDEVICE when no MI355X is visible.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ARMOUR_KEY128=1 selects the second ABI of include/armour_types.h for the whole process: libarmour_hip_k128.so (128-bit monomial keys, 8 factors)
KEY128 = os.environ.get("ARMOUR_KEY128", "0") not in ("", "0")
LIB_PATH = os.environ.get("ARMOUR_HIP_LIB") or os.path.join(_HERE, "lib", "libarmour_hip_k128.so" if KEY128 else "libarmour_hip.so")  # env override: A/B builds

MAXJ = 9                    # ARMOUR_MAX_JOINTS
MAXF = 8 if KEY128 else 7   # ARMOUR_MAX_FACTORS (checked against armour_abi_max_factors() of the library that was loaded)
KEY_WORDS = 2 if KEY128 else 1   # u64 words of a monomial key as the one-operator hook passes it, low word first (sizeof(pzkey_t) / 8)


def keys_to_words(keys):
    """Monomial keys -> contiguous [n, KEY_WORDS] u64 array.  keys: Python integers (a list, or an array of them), a u64 array, or [n, KEY_WORDS] already."""
    a = np.asarray(keys)
    if a.ndim == 2:
        assert a.shape[1] == KEY_WORDS, (a.shape, KEY_WORDS)
        return np.ascontiguousarray(a, dtype=np.uint64)
    out = np.zeros((len(a), KEY_WORDS), np.uint64)
    for i, k in enumerate(a.tolist()):
        k = int(k)
        assert 0 <= k < 1 << (64 * KEY_WORDS), "key does not fit the library's key width"
        for w in range(KEY_WORDS):
            out[i, w] = (k >> (64 * w)) & 0xFFFFFFFFFFFFFFFF
    return out


def words_to_keys(words):
    """[n, KEY_WORDS] u64 -> keys: a u64 array with one word per key (as ever), an object array of Python integers with two."""
    if KEY_WORDS == 1:
        return np.ascontiguousarray(words[:, 0])
    out = np.empty(len(words), dtype=object)
    for i in range(len(words)):
        out[i] = sum(int(words[i, w]) << (64 * w) for w in range(KEY_WORDS))
    return out


OK, EINVAL, EDEVICE, ECAPACITY, ESTATE = 0, -1, -2, -3, -4
ROADMAP_KNN_MAX = 64         # ARMOUR_ROADMAP_KNN_MAX
ROADMAP_KNN_MANY = 2048      # ARMOUR_ROADMAP_KNN_MANY: from this many queries on the search takes a lane per query
TREE_NOT_FOUND, TREE_FOUND, TREE_START_BLOCKED, TREE_GOAL_BLOCKED, TREE_FULL = 0, 1, 2, 3, 4   # ARMOUR_TREE_*
TREE_MAX_NODES, TREE_MAX_ITERATIONS = 8192, 100000   # ARMOUR_TREE_MAX_NODES, ARMOUR_TREE_MAX_ITERATIONS
SHORTCUT_OK, SHORTCUT_INVALID = 0, 1                 # ARMOUR_SHORTCUT_*
SHORTCUT_MAX_POINTS, SHORTCUT_MAX_PASSES = 1024, 8   # ARMOUR_SHORTCUT_MAX_POINTS, ARMOUR_SHORTCUT_MAX_PASSES
IK_NONE_CONVERGED, IK_FOUND, IK_ALL_BLOCKED = 0, 1, 2   # ARMOUR_IK_*
IK_MAX_SEEDS, IK_MAX_ITERATIONS, IK_MAX_TARGETS = 256, 1000, 1048576   # ARMOUR_IK_MAX_SEEDS, ARMOUR_IK_MAX_ITERATIONS, ARMOUR_IK_MAX_TARGETS
WS_PARTIAL, WS_REACHED, WS_START_BLOCKED = 0, 1, 2      # ARMOUR_WS_*
WS_MAX_NODES, WS_MAX_SEGMENTS = 4096, 1024              # ARMOUR_WS_MAX_NODES, ARMOUR_WS_MAX_SEGMENTS


class ArmourRobot(C.Structure):
    _fields_ = [
        ("num_joints", C.c_int32), ("num_factors", C.c_int32),
        ("axes", C.c_int32 * MAXJ), ("continuous", C.c_int32 * MAXF),
        ("trans", C.c_double * ((MAXJ + 1) * 3)), ("rots", C.c_double * (MAXJ * 3)),
        ("mass", C.c_double * MAXJ), ("mass_uncertainty", C.c_double),
        ("com", C.c_double * (MAXJ * 3)),
        ("inertia", C.c_double * (MAXJ * 9)), ("inertia_uncertainty", C.c_double),
        ("friction", C.c_double * MAXJ), ("damping", C.c_double * MAXJ), ("armature", C.c_double * MAXJ),
        ("state_limits_lb", C.c_double * MAXF), ("state_limits_ub", C.c_double * MAXF),
        ("speed_limits", C.c_double * MAXF), ("torque_limits", C.c_double * MAXF),
        ("gravity", C.c_double),
        ("link_zonotope_center", C.c_double * (MAXJ * 3)), ("link_zonotope_generators", C.c_double * (MAXJ * 3)),
        ("alpha", C.c_double), ("V_m", C.c_double), ("M_max", C.c_double), ("M_min", C.c_double), ("K", C.c_double),
        ("mass_uncertainty_link", C.c_double * MAXJ), ("inertia_uncertainty_link", C.c_double * MAXJ),
    ]


class ArmourParams(C.Structure):
    _fields_ = [
        ("num_time_steps", C.c_int32), ("input_constraints_off", C.c_int32),
        ("duration", C.c_double), ("k_range", C.c_double * MAXF),
        ("simplify_threshold", C.c_double), ("t_plan", C.c_double), ("cost_scale", C.c_double),
        ("collision_violation_threshold", C.c_double), ("torque_violation_threshold", C.c_double),
    ]


class ArmourLimits(C.Structure):
    _fields_ = [
        ("max_batch", C.c_int32), ("max_obstacles", C.c_int32), ("link_monomials", C.c_int32),
        ("torque_monomials", C.c_int32), ("work_monomials", C.c_int32), ("raw_terms", C.c_int32),
    ]


class ArmourSolveOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("max_line_search", C.c_int32), ("tolerance", C.c_double),
                ("max_wall_time_s", C.c_double), ("force_host_qp", C.c_double), ("reserved", C.c_double * 3)]


class ArmourSolveResult(C.Structure):
    _fields_ = [("k_opt", C.c_double * MAXF), ("cost", C.c_double), ("max_violation", C.c_double), ("feasible", C.c_int32),
                ("iterations", C.c_int32), ("evaluations", C.c_int32), ("status", C.c_int32), ("time_ms", C.c_double)]


class ArmourTrackOptions(C.Structure):
    _fields_ = [("controller", C.c_int32), ("record_every", C.c_int32), ("steps_per_launch", C.c_int32), ("reserved0", C.c_int32),
                ("Kr", C.c_double * MAXF), ("alpha", C.c_double), ("V_max", C.c_double), ("r_norm_threshold", C.c_double),
                ("model_uncertainty", C.c_double), ("dt", C.c_double), ("t0", C.c_double), ("t1", C.c_double), ("duration", C.c_double),
                ("althoff_Kp", C.c_double * 2), ("reserved", C.c_double * 2)]


class ArmourTrackResult(C.Structure):
    _fields_ = [("status", C.c_int32), ("steps", C.c_int32), ("limit_flags", C.c_int32), ("reserved", C.c_int32),
                ("t_end", C.c_double), ("q", C.c_double * MAXF), ("qd", C.c_double * MAXF),
                ("max_pos_error", C.c_double), ("max_vel_error", C.c_double), ("max_V", C.c_double), ("max_robust_input", C.c_double),
                ("max_torque_ratio", C.c_double), ("first_violation_t", C.c_double)]


TRACK_CTL_ROBUST, TRACK_CTL_NOMINAL, TRACK_CTL_NONE, TRACK_CTL_ALTHOFF = 0, 1, 2, 4   # ARMOUR_TRACK_CTL_* (3 is unassigned)
TRACK_LIMIT_TORQUE, TRACK_LIMIT_POSITION, TRACK_LIMIT_SPEED = 1, 2, 4   # ARMOUR_TRACK_LIMIT_*


class ArmourViolation(C.Structure):
    _fields_ = [("l1_violation", C.c_double), ("worst", C.c_double), ("worst_row", C.c_int32), ("n_violated", C.c_int32),
                ("n_outside_slack", C.c_int32), ("feasible", C.c_int32)]


class ArmourSweepRecord(C.Structure):   # armour_sweep: the violation record of one candidate and its cost (40 bytes)
    _fields_ = [("v", ArmourViolation), ("cost", C.c_double)]


SWEEP_MAX_CANDIDATES = 4096   # ARMOUR_SWEEP_MAX_CANDIDATES

OPT_P1_BUILD = 1   # ARMOUR_OPT_P1_BUILD: 0 automatic, 1 per time step, 2 time-vectorised
OPT_P1_WORK_MEMORY_MB = 2   # ARMOUR_OPT_P1_WORK_MEMORY_MB: cap on the time-vectorised build's work memory, MiB (0: none)
# the other per-handle options of include/armour_hip.h (launch shapes: bit-identical keys / coefficients / centres for every value)
OPT_P1_KEEP_WORK_MEMORY = 3
OPT_P1_STEP_WAVES = 101
OPT_P1_STEP_FREE = 102
OPT_P1_STEP_SPLIT_FK = 103
OPT_P1_STEP_AUX3 = 104
OPT_P1_MAX_WAVES_PER_CU = 105
OPT_P1_TWO_PASS = 106
OPT_P1_STEP_PAIRS = 107
OPT_P1_STEP_QUEUE = 109
OPT_P1_STEP_TAIL_CROSS = 108
OPT_P1_STEP_TWO_CU = 123     # 3 (default) | 0..2: a lone problem's time step on two compute units (include/armour_hip.h); 10 + level: the fall-back's test hook
OPT_P1_STEP_LEAN_BACK = 124  # 1 (default) | 0: with level 3, the backward pass's f-recursion on the helper block as well
OPT_P1_TV_TAIL_CROSS = 121
OPT_P1_TV_MIN_GROUPS = 110
OPT_P1_TV_WAVES = 111
OPT_P1_TV_FREE = 112
OPT_P1_TV_SPLIT_FK = 113
OPT_P1_TV_DEDICATED = 114
OPT_P1_TV_HELP_SHIFT = 115
OPT_P1_TV_HELPERS = 116
OPT_P1_TV_HELP_MIN = 117
OPT_P1_TV_HELP_N = 118
OPT_P1_TV_AUX3 = 119
OPT_P1_FULL_PLANES = 120
OPT_P1_TV_ROW_WIDTH = 122   # 0 automatic | 50 | 64 doubles per row of the time-vectorised kernel's work slots
OPT_P2_EX = 130
OPT_P2_NO_ZERO_TEST = 134   # 0: the EX kernels keep the scan's zero-normal test (armour_debug_p2_zero_plan says which form a handle takes)
OPT_STEPS_GRAPH_MIN = 131
OPT_PINNED_MODE = 132
OPT_CULL_ROWS = 133   # 1: armour_eval_violations* evaluate only the rows that can be violated for some k (armour_get_row_relevance)
OPT_SOLVE_SUB_TILES = 140
OPT_SOLVE_DEVICE = 141
OPT_SOLVE_CUT_TILES = 142
OPT_SOLVE_BLOCKS = 143
OPT_SOLVE_SUB_BATCH = 144
OPT_SOLVE_ROW_CAP = 145
OPT_SOLVE_HARD_CAP_S = 146
OPT_SOLVE_WAVES_PER_SIMD = 147
OPT_SOLVE_CULL = 148   # -1 automatic | 0 | 1: the device-resident solve walks only the rows that can ever be QP candidates (same iterates)

# every symbol include/armour_hip.h declares (tests check the .so exports all of them)
EXPORTS = [
    "armour_robot_kinova_gen3_no_gripper", "armour_robot_kinova_gen3_gripper", "armour_robot_fetch", "armour_robot_fetch8", "armour_params_default", "armour_create", "armour_destroy",
    "armour_last_error", "armour_device_available", "armour_alloc_pinned", "armour_free_pinned", "armour_set_problems", "armour_set_problems_armtd", "armour_get_sizes",
    "armour_get_bounds", "armour_eval_f", "armour_eval_grad_f", "armour_eval_g_jac",
    "armour_eval_g_jac_device", "armour_eval_g_jac_device_steps", "armour_prepare_steps", "armour_eval_g_jac_device_multi", "armour_desired_trajectory", "armour_robust_controller", "armour_althoff_controller", "armour_check_feasible", "armour_get_torque_radius",
    "armour_get_link_generators", "armour_get_link_centers", "armour_get_pz", "armour_get_table_sizes",
    "armour_solve_options_default", "armour_solve", "armour_debug_qp", "armour_debug_qp_box", "armour_debug_qp_elastic", "armour_debug_qp_device", "armour_debug_pz_op",
    "armour_get_hyperplanes", "armour_get_build_ms", "armour_get_build_info", "armour_p2_kernel_name", "armour_debug_load_tables",
    "armour_get_plane_skip", "armour_get_prune_margin", "armour_batch_get_prune_margin", "armour_set_option", "armour_get_option", "armour_controller_set_kernel", "armour_device_memory", "armour_abi_max_factors", "armour_eval_violations_device", "armour_eval_violations", "armour_get_row_relevance", "armour_get_solver_rows", "armour_debug_get_row_lists",
    "armour_batch_partition", "armour_batch_create", "armour_batch_destroy", "armour_batch_set_option", "armour_batch_set_problems",
    "armour_batch_get_sizes", "armour_batch_get_bounds", "armour_batch_eval_g_jac", "armour_batch_eval_violations", "armour_batch_solve",
    "armour_batch_get_build_ms", "armour_batch_get_build_info",
    "armour_roadmap_create", "armour_roadmap_destroy", "armour_roadmap_get_sizes", "armour_roadmap_check", "armour_roadmap_plan",
    "armour_track_options_default", "armour_track", "armour_track_auto_steps",
    "armour_path_audit", "armour_path_audit_host", "armour_path_audit_items",
    "armour_set_problems_moving", "armour_path_audit_moving", "armour_path_audit_moving_host",
    "armour_solve_from", "armour_sweep", "armour_sweep_tile",
    "armour_self_pairs_default", "armour_self_check", "armour_self_check_host", "armour_self_edges_host", "armour_roadmap_check_self",
    "armour_roadmap_use_self", "armour_path_audit_self", "armour_path_audit_self_host",
    "armour_roadmap_field", "armour_roadmap_descend",
    "armour_roadmap_check_moving", "armour_roadmap_check_moving_host",
    "armour_roadmap_check_slices", "armour_roadmap_check_slices_host", "armour_roadmap_arrival", "armour_roadmap_arrival_host",
    "armour_roadmap_create_host", "armour_roadmap_knn", "armour_roadmap_knn_host", "armour_roadmap_connect_batch", "armour_roadmap_descend_batch",
    "armour_tree_plan", "armour_tree_plan_host", "armour_path_shortcut", "armour_path_shortcut_host",
    "armour_tree_plan_moving", "armour_tree_plan_moving_host", "armour_path_shortcut_moving", "armour_path_shortcut_moving_host",
    "armour_ik", "armour_ik_host", "armour_ik_end_effector_host", "armour_ik_moving", "armour_ik_moving_host",
    "armour_ws_tree_plan", "armour_ws_tree_plan_host", "armour_ws_tree_plan_moving", "armour_ws_tree_plan_moving_host",
    "armour_ws_trees_create", "armour_ws_trees_create_host", "armour_ws_trees_destroy", "armour_ws_trees_grow", "armour_ws_trees_read",
    "armour_debug_ws_trees_set_iterations",
    "armour_debug_block_steps", "armour_debug_block_split", "armour_debug_block_owner",
    "armour_debug_p2_plan", "armour_debug_p2_plan_shape", "armour_debug_p2_zero_plan", "armour_debug_p2_zero_plan_shape",
]

_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  The PyTorch-ROCm wheel bundles its own libamdhip64.so (SONAME libamdhip64.so.7,
    the name libarmour_hip.so links against) but refers to it by file name, so if libarmour_hip.so pulled in
    /opt/rocm's copy first a later `import torch` would load a second runtime next to it, and device discovery in
    the second one fails ("no ROCm-capable device is detected").  When torch is installed, map its copy first (no
    torch import needed): the dynamic linker then binds libarmour_hip.so to it by SONAME and torch finds it already
    loaded.  Without torch nothing happens and /opt/rocm's runtime is used."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load():
    """Load libarmour_hip.so (raises OSError with build instructions if it is absent)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError(
            f"{LIB_PATH} not found: build it with `make -C armour_amd/csrc` (hipcc, gfx950) or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU path.")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    if hasattr(L, "armour_abi_max_factors") and L.armour_abi_max_factors() != MAXF:
        raise RuntimeError(f"{LIB_PATH} is built for {L.armour_abi_max_factors()} factors, this process mirrors its structs for {MAXF} (ARMOUR_KEY128)")
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    vp = C.c_void_p
    L.armour_robot_kinova_gen3_no_gripper.argtypes = [C.POINTER(ArmourRobot)]
    L.armour_robot_kinova_gen3_no_gripper.restype = None
    L.armour_robot_kinova_gen3_gripper.argtypes = [C.POINTER(ArmourRobot)]
    L.armour_robot_fetch.argtypes = [C.POINTER(ArmourRobot)]
    L.armour_robot_fetch.restype = None
    L.armour_robot_fetch8.argtypes = [C.POINTER(ArmourRobot)]
    L.armour_robot_fetch8.restype = C.c_int
    L.armour_robot_kinova_gen3_gripper.restype = None
    L.armour_params_default.argtypes = [C.POINTER(ArmourParams), C.c_int32]
    L.armour_params_default.restype = None
    L.armour_create.argtypes = [C.POINTER(ArmourRobot), C.POINTER(ArmourParams), C.POINTER(ArmourLimits), C.c_int32, C.POINTER(vp)]
    L.armour_destroy.argtypes = [vp]
    L.armour_destroy.restype = None
    L.armour_last_error.restype = C.c_char_p
    L.armour_alloc_pinned.argtypes = [C.c_uint64, C.POINTER(vp)]
    L.armour_free_pinned.argtypes = [vp]
    L.armour_free_pinned.restype = None
    L.armour_set_problems.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp]
    if hasattr(L, "armour_set_problems_moving"):   # (absent from a library of an earlier commit selected with ARMOUR_HIP_LIB for a comparison)
        L.armour_set_problems_moving.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp]
    L.armour_set_problems_armtd.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp, dp]
    L.armour_get_sizes.argtypes = [vp, ip, ip, ip]
    L.armour_get_bounds.argtypes = [vp, dp, dp, dp, dp]
    L.armour_eval_f.argtypes = [vp, dp, dp]
    L.armour_eval_grad_f.argtypes = [vp, dp, dp]
    L.armour_eval_g_jac.argtypes = [vp, dp, dp, dp]
    L.armour_eval_g_jac_device.argtypes = [vp, vp, vp, vp, vp]
    L.armour_eval_g_jac_device_steps.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
    L.armour_prepare_steps.argtypes = [vp, vp, C.c_int32, vp, vp]
    L.armour_eval_g_jac_device_multi.argtypes = [vp, vp, C.c_int32, vp, vp, vp]
    L.armour_desired_trajectory.argtypes = [C.c_int32, dp, dp, dp, dp, C.c_double, dp, C.c_double, dp, dp, dp]
    L.armour_robust_controller.argtypes = [C.POINTER(ArmourRobot), C.c_double, dp, C.c_double, C.c_double, C.c_double, C.c_int32, dp, dp, dp, dp, dp, dp, dp, dp]
    L.armour_althoff_controller.argtypes = [C.POINTER(ArmourRobot), C.c_double, dp, dp, dp, dp, C.c_int32, dp, dp, dp, dp, dp, dp, dp, dp]
    L.armour_check_feasible.argtypes = [vp, dp, ip]
    L.armour_solve_options_default.argtypes = [C.POINTER(ArmourSolveOptions)]
    L.armour_solve_options_default.restype = None
    L.armour_solve.argtypes = [vp, C.POINTER(ArmourSolveOptions), C.POINTER(ArmourSolveResult)]
    L.armour_solve_from.argtypes = [vp, C.POINTER(ArmourSolveOptions), dp, C.POINTER(ArmourSolveResult)]
    L.armour_sweep.argtypes = [vp, C.c_int32, dp, C.c_int32, C.POINTER(ArmourSweepRecord), ip, dp]
    L.armour_sweep_tile.argtypes = []
    L.armour_debug_qp.argtypes = [C.c_int32, dp, dp, C.c_int32, dp, dp, dp, dp, ip]
    L.armour_debug_qp_box.argtypes = [C.c_int32, dp, dp, C.c_int32, dp, dp, dp, dp, dp, C.c_int32, dp, ip, ip, dp]
    L.armour_debug_qp_elastic.argtypes = [C.c_int32, dp, dp, dp, C.c_int32, dp, dp, dp, ip, ip, dp, ip, ip, ip, ip, ip]
    L.armour_debug_qp_device.argtypes = [C.c_int32, dp, dp, dp, C.c_int32, dp, dp, C.c_int32, C.c_int32, dp, ip, ip, dp, ip]
    L.armour_debug_pz_op.argtypes = [vp, C.c_int32, C.c_int32, ip, ip, C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(dp), dp, dp, dp, dp,
                                     C.c_int32, C.c_int32, C.POINTER(C.c_uint64), dp, dp, C.c_int32, C.c_int32]
    L.armour_get_torque_radius.argtypes = [vp, dp]
    L.armour_get_link_generators.argtypes = [vp, dp]
    L.armour_get_link_centers.argtypes = [vp, dp, dp]
    L.armour_get_pz.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, C.POINTER(C.c_uint64), dp, C.c_int32]
    L.armour_get_table_sizes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.armour_get_hyperplanes.argtypes = [vp, dp, dp, dp]
    L.armour_get_build_ms.argtypes = [vp, dp]
    L.armour_get_build_info.argtypes = [vp, ip]
    L.armour_p2_kernel_name.restype = C.c_char_p
    L.armour_debug_load_tables.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, ip, dp, C.POINTER(C.c_uint64), dp,
                                           C.c_int32, ip, dp, C.POINTER(C.c_uint64), dp, C.c_int32, dp, dp, dp, dp]
    L.armour_get_plane_skip.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.armour_get_prune_margin.argtypes = [vp, dp]
    L.armour_batch_get_prune_margin.argtypes = [vp, dp]
    L.armour_set_option.argtypes = [vp, C.c_int32, C.c_double]
    L.armour_get_option.argtypes = [vp, C.c_int32, dp]
    L.armour_device_memory.argtypes = [C.c_int32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.armour_controller_set_kernel.argtypes = [C.c_int32]
    L.armour_eval_violations_device.argtypes = [vp, vp, vp, vp]
    L.armour_eval_violations.argtypes = [vp, dp, C.POINTER(ArmourViolation)]
    L.armour_get_row_relevance.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.armour_get_solver_rows.argtypes = [vp, C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]
    L.armour_debug_get_row_lists.argtypes = [vp, C.c_int32, ip, ip, ip, ip, C.POINTER(C.c_int64), dp, C.c_int64, C.POINTER(C.c_int64)]
    L.armour_batch_partition.argtypes = [C.c_int32, C.c_int32, ip]
    L.armour_batch_create.argtypes = [C.POINTER(ArmourRobot), C.POINTER(ArmourParams), C.POINTER(ArmourLimits), ip, C.c_int32, C.POINTER(vp)]
    L.armour_batch_destroy.argtypes = [vp]
    L.armour_batch_destroy.restype = None
    L.armour_batch_set_option.argtypes = [vp, C.c_int32, C.c_double]
    L.armour_batch_set_problems.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, dp]
    L.armour_batch_get_sizes.argtypes = [vp, ip, ip, ip, ip]
    L.armour_batch_get_bounds.argtypes = [vp, dp, dp, dp, dp]
    L.armour_batch_eval_g_jac.argtypes = [vp, dp, dp, dp]
    L.armour_batch_eval_violations.argtypes = [vp, dp, C.POINTER(ArmourViolation)]
    L.armour_batch_solve.argtypes = [vp, C.POINTER(ArmourSolveOptions), C.POINTER(ArmourSolveResult)]
    L.armour_batch_get_build_ms.argtypes = [vp, dp, dp]
    L.armour_batch_get_build_info.argtypes = [vp, ip]
    u8p = C.POINTER(C.c_uint8)
    L.armour_roadmap_create.argtypes = [C.POINTER(ArmourRobot), C.c_int32, dp, C.c_int32, ip, u8p, C.c_double, C.c_int32, C.POINTER(vp)]
    L.armour_roadmap_destroy.argtypes = [vp]
    L.armour_roadmap_destroy.restype = None
    L.armour_roadmap_get_sizes.argtypes = [vp, ip, ip, C.POINTER(C.c_int64)]
    L.armour_roadmap_check.argtypes = [vp, C.c_int32, C.c_int32, dp, u8p, u8p, dp, dp]
    if hasattr(L, "armour_roadmap_check_moving"):   # (absent from a library of an earlier commit selected with ARMOUR_HIP_LIB for a comparison)
        L.armour_roadmap_check_moving.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, u8p, u8p, dp, dp]
        L.armour_roadmap_check_moving_host.argtypes = [vp, C.c_int32, C.c_int32, dp, dp, dp, dp, u8p, u8p, dp]
    if hasattr(L, "armour_roadmap_check_slices"):   # (absent from a library of an earlier commit selected with ARMOUR_HIP_LIB for a comparison)
        u64p = C.POINTER(C.c_uint64)
        slices = [vp, C.c_int32, C.c_int32, dp, dp, dp, C.c_double, C.c_int32, C.c_int32, ip, dp, dp, u64p, u64p, u64p, dp]
        arrival = [vp, C.c_double, C.c_int32, ip, ip, ip, dp, u64p, u64p, u64p, u64p, ip, ip, ip, ip, ip]
        L.armour_roadmap_check_slices.argtypes = slices + [dp]
        L.armour_roadmap_check_slices_host.argtypes = slices
        L.armour_roadmap_arrival.argtypes = arrival + [dp]
        L.armour_roadmap_arrival_host.argtypes = arrival
    L.armour_roadmap_plan.argtypes = [vp, C.c_int32, dp, dp, C.c_int32, C.c_int32, dp, ip]
    L.armour_roadmap_field.argtypes = [vp, dp, C.c_int32, dp, ip, ip, ip, dp]
    L.armour_roadmap_descend.argtypes = [vp, C.c_int32, dp, C.c_int32, C.c_int32, dp, ip, dp]
    L.armour_roadmap_create_host.argtypes = [C.POINTER(ArmourRobot), C.c_int32, dp, C.c_int32, ip, u8p, C.c_double, C.POINTER(vp)]
    knn = [vp, C.c_int32, dp, ip, ip, C.c_int32, C.c_double, ip, dp, ip, dp]
    L.armour_roadmap_knn.argtypes = knn
    L.armour_roadmap_knn_host.argtypes = knn
    L.armour_roadmap_connect_batch.argtypes = [vp, C.c_int32, ip, dp, dp, C.c_int32, ip, dp, u8p, ip, u8p, dp]
    L.armour_roadmap_descend_batch.argtypes = [vp, C.c_int32, ip, dp, C.c_int32, C.c_int32, ip, ip, u8p, dp]
    tree = [C.POINTER(ArmourRobot), u8p, dp, dp, C.c_int32, C.c_int32, dp, dp, dp, C.POINTER(C.c_uint64), C.c_double, C.c_double, C.c_int32, C.c_int32,
            C.c_int32, ip, ip, ip, dp, ip, dp, ip, dp]
    L.armour_tree_plan.argtypes = tree            # (the last pointer: ms)
    L.armour_tree_plan_host.argtypes = tree       # (the last pointer: margin [W])
    short = [C.POINTER(ArmourRobot), u8p, C.c_int32, C.c_int32, dp, C.c_int32, dp, ip, C.c_double, C.c_int32, C.c_int32, ip, ip, ip, ip, dp, dp, dp, dp]
    L.armour_path_shortcut.argtypes = short       # (the last pointer: ms)
    L.armour_path_shortcut_host.argtypes = short  # (the last pointer: margin [W])
    if hasattr(L, "armour_tree_plan_moving"):   # (absent from a library of an earlier commit selected with ARMOUR_HIP_LIB for a comparison)
        L.armour_tree_plan_moving.argtypes = L.armour_tree_plan_moving_host.argtypes = tree[:7] + [dp, dp, dp] + tree[7:]         # velocity, t_from, t_to
        L.armour_path_shortcut_moving.argtypes = L.armour_path_shortcut_moving_host.argtypes = short[:5] + [dp, dp, dp] + short[5:]
    ik = [C.POINTER(ArmourRobot), u8p, dp, dp, dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, dp, ip, dp, dp, C.POINTER(C.c_uint64), C.c_double, C.c_double,
          C.c_double, C.c_int32, ip, ip, dp, dp, dp, ip, ip, dp]
    L.armour_ik.argtypes = ik                     # (the last pointer: ms)
    L.armour_ik_host.argtypes = ik                # (the last pointer: margin [N])
    L.armour_ik_end_effector_host.argtypes = [C.POINTER(ArmourRobot), C.c_int32, dp, dp, dp, dp]
    ws = [dp, dp, C.c_int32, C.c_int32, dp, dp, dp, C.POINTER(C.c_uint64), C.c_int32, dp, ip] + [C.c_double] * 6 + [C.c_int32] * 3 + [ip] * 5 + [
        dp, dp, dp, ip, dp, ip, dp, dp]
    L.armour_ws_tree_plan.argtypes = ws           # (the last pointer: ms)
    L.armour_ws_tree_plan_host.argtypes = ws      # (the last pointer: margin [W])
    if hasattr(L, "armour_ws_tree_plan_moving"):   # (absent from a library of an earlier commit selected with ARMOUR_HIP_LIB for a comparison)
        L.armour_ik_moving.argtypes = L.armour_ik_moving_host.argtypes = ik[:10] + [dp, dp, dp] + ik[10:]                         # velocity, t_from, t_to
        L.armour_ws_tree_plan_moving.argtypes = L.armour_ws_tree_plan_moving_host.argtypes = ws[:5] + [dp, dp, dp] + ws[5:]
    if hasattr(L, "armour_ws_trees_create"):   # (absent from a library of an earlier commit selected with ARMOUR_HIP_LIB for a comparison)
        trees = [dp, dp, C.c_int32, C.c_int32, dp, dp, C.POINTER(C.c_uint64)] + [C.c_double] * 6 + [C.c_int32, C.POINTER(vp)]
        L.armour_ws_trees_create.argtypes = trees
        L.armour_ws_trees_create_host.argtypes = trees
        L.armour_ws_trees_destroy.argtypes = [vp]
        L.armour_ws_trees_destroy.restype = None
        L.armour_ws_trees_grow.argtypes = [vp, C.c_int32, ip, dp, C.c_int32, C.c_int32, ip, ip, ip, ip, dp, dp, dp, ip, dp, dp]
        L.armour_ws_trees_read.argtypes = [vp, C.c_int32, ip, dp, ip, dp, ip]
        L.armour_debug_ws_trees_set_iterations.argtypes = [vp, C.c_int32, C.c_int32]
    L.armour_debug_block_steps.argtypes = [dp, ip, ip, ip, dp, ip, ip, ip, ip, ip]
    L.armour_debug_block_split.argtypes = [C.c_int32, C.c_int32, C.c_int32, ip]
    L.armour_debug_block_owner.argtypes = [ip, C.c_int32, C.c_int32, ip, ip]
    if hasattr(L, "armour_debug_p2_plan"):   # (absent from a library of an earlier commit selected with ARMOUR_HIP_LIB for a comparison)
        L.armour_debug_p2_plan.argtypes = [vp, ip, C.POINTER(C.c_uint32)]
        L.armour_debug_p2_plan_shape.argtypes = [C.c_int32] * 8 + [C.POINTER(C.c_uint64), ip, C.POINTER(C.c_uint32)]
    if hasattr(L, "armour_debug_p2_zero_plan"):
        L.armour_debug_p2_zero_plan.argtypes = [vp, ip, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.armour_debug_p2_zero_plan_shape.argtypes = [C.c_int32] * 8 + [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), ip]
    L.armour_track_options_default.argtypes = [C.POINTER(ArmourRobot), C.POINTER(ArmourTrackOptions)]
    L.armour_track_options_default.restype = None
    L.armour_track.argtypes = [C.POINTER(ArmourRobot), C.POINTER(ArmourTrackOptions), C.c_int32, dp, dp, dp, dp, dp, dp, dp, dp,
                               C.POINTER(ArmourTrackResult), dp, dp]
    L.armour_track_auto_steps.argtypes = [C.c_int32]
    audit = [C.POINTER(ArmourRobot), C.c_int32, C.c_int32, dp, C.c_int32, ip, dp, dp, dp, dp, dp, C.c_double, dp, dp, dp, C.c_double, ip, dp, dp]
    L.armour_path_audit.argtypes = audit + [dp]
    L.armour_path_audit_host.argtypes = audit
    audit_moving = [C.POINTER(ArmourRobot), C.c_int32, C.c_int32, dp, dp, C.c_int32, ip, dp, dp, dp, dp, dp, dp, C.c_double, dp, dp, dp, C.c_double, ip, dp, dp]
    if hasattr(L, "armour_path_audit_moving"):
        L.armour_path_audit_moving.argtypes = audit_moving + [dp]
        L.armour_path_audit_moving_host.argtypes = audit_moving
    L.armour_path_audit_items.argtypes = [C.POINTER(ArmourRobot), C.c_int32, dp, dp, dp, dp, dp, C.c_double, dp, dp, C.c_double, C.POINTER(C.c_int64)]
    rp = C.POINTER(ArmourRobot)
    L.armour_self_pairs_default.argtypes = [rp, u8p]
    L.armour_self_check.argtypes = [rp, u8p, dp, C.c_int32, dp, u8p, dp, ip, dp]
    L.armour_self_check_host.argtypes = [rp, u8p, dp, C.c_int32, dp, u8p, dp, ip]
    L.armour_self_edges_host.argtypes = [rp, u8p, C.c_double, u8p, dp, C.c_int32, dp, dp, u8p]
    L.armour_roadmap_check_self.argtypes = [vp, u8p, dp, u8p, u8p, dp, dp]
    L.armour_roadmap_use_self.argtypes = [vp, C.c_int32]
    audit_self = [rp, u8p, dp, C.c_int32, dp, dp, dp, dp, dp, C.c_double, dp, dp, dp, C.c_double, ip, dp, dp]
    L.armour_path_audit_self.argtypes = audit_self + [dp]
    L.armour_path_audit_self_host.argtypes = audit_self
    _lib = L
    return L


class ArmourError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"armour error {code}: {msg}")
        self.code = code


def _dp(a):
    """A float64 array as the double* the C ABI takes (None: a null pointer)."""
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def check(rc):
    if rc < 0:
        raise ArmourError(rc, load().armour_last_error().decode())
    return rc


def as_worlds(obstacles):
    """obstacles [W,O,12] (or [O,12]: W = 1) -> (the contiguous float64 array [W,O,12], W, O), as every entry with worlds takes them."""
    obs = np.asarray(obstacles, dtype=np.float64)
    obs = np.ascontiguousarray(obs.reshape((1,) + obs.shape) if obs.ndim == 2 else obs)
    return obs, obs.shape[0], obs.shape[1]


class Result:
    """What a wrapper returns: its keyword arguments as attributes (the wrappers' result classes say which)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
