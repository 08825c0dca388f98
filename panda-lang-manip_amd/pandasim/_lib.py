"""ctypes binding of libpandasim.so (include/pandasim.h).

The library is built in-tree (``python -m pandasim.build`` or
``__graft_entry__.build()``) and loaded from this package directory.  There is
no CPU fallback: if the library or a GPU is missing, calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PANDASIM_LIB", os.path.join(HERE, "libpandasim.so"))

PS_OK = 0
PS_MAX_UNIFORM = 8
ERRORS = {-1: "PS_ERR_ARG", -2: "PS_ERR_HIP", -3: "PS_ERR_UNSUPPORTED"}

# float row indices of the SoA state (include/pandasim.h)
F_Q, F_QD, F_MTARGET, F_MKP, F_MKD, F_MVEL, F_MIMP = 0, 9, 18, 27, 36, 45, 54
F_CPOS, F_CQUAT, F_CVEL, F_COMG = 63, 66, 70, 73
F_C2POS, F_C2QUAT, F_C2VEL, F_C2OMG = 76, 79, 83, 86
OBJECT_ROWS = (F_CPOS, F_C2POS)  # pos, quat (+3), vel (+7), omg (+10) of object 0 / 1
# warm-start contact cache (ground of object 0 / 1, gripper, object-object)
F_WG0, F_WG0ID, F_WG1, F_WG1ID, F_WR, F_WRID, F_WP, F_WPPT, F_WPN = 89, 93, 94, 98, 99, 103, 104, 108, 120
NUM_FLOAT_ROWS = 121
NUM_RNG_ROWS = 5
MAX_GOAL_DIM = 6
SHAPE_BOX, SHAPE_CYLINDER = 0, 1


class Config(C.Structure):
    _fields_ = [
        ("task", C.c_int32), ("control", C.c_int32), ("reward", C.c_int32), ("block_gripper", C.c_int32),
        ("has_table", C.c_int32), ("has_plane", C.c_int32), ("n_objects", C.c_int32), ("object_shape", C.c_int32),
        ("base", C.c_float * 3), ("object_half", C.c_float * 3),
        ("object_mass", C.c_float), ("object2_mass", C.c_float), ("object_friction", C.c_float),
        ("table_cx", C.c_float), ("table_hx", C.c_float), ("table_hy", C.c_float),
    ]


class Visual(C.Structure):
    """ps_visual (include/pandasim.h): colours by role and ghost-target shapes."""
    _fields_ = [("rgba", (C.c_float * 4) * 8), ("target_shape", C.c_int32 * 2), ("target_half", (C.c_float * 3) * 2)]


class CloudView(C.Structure):
    """ps_cloud_view: one view of ps_point_cloud, as ps_camera returns it."""
    _fields_ = [("view", C.c_float * 16), ("proj", C.c_float * 16), ("tran_pix_world", C.c_double * 16)]


class CloudScale(C.Structure):
    """ps_cloud_scale: one radius of ps_cloud_set_abstraction (device pointers)."""
    _fields_ = [("radius", C.c_double), ("nsample", C.c_int32), ("group_idx", C.c_void_p), ("grouped", C.c_void_p)]


class CloudMlpLayer(C.Structure):
    """ps_cloud_mlp_layer: W [c_out, c_in] and b [c_out] (device pointers)."""
    _fields_ = [("W", C.c_void_p), ("b", C.c_void_p), ("c_out", C.c_int32), ("relu", C.c_int32)]


class CloudMlpBfloatLayer(C.Structure):
    """ps_cloud_mlp_bfloat_layer: W [c_out, ldw] bf16 bits (ldw = c_in rounded up to
    a multiple of 8, 16-byte aligned) and b [c_out] f32 (device pointers)."""
    _fields_ = [("W", C.c_void_p), ("b", C.c_void_p), ("c_out", C.c_int32), ("relu", C.c_int32)]


class CloudCrop(C.Structure):
    """ps_cloud_crop: the open box lo < p < hi on the world point."""
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3)]


VISUAL_SPHERE = 2
ROLES = ("plane", "table", "object1", "object2", "target1", "target2", "robot", "background")


class ReplayLayout(C.Structure):
    """ps_replay_layout: byte offsets into the replay buffer, word offsets into a row."""
    _fields_ = ([(n, C.c_int64) for n in ("bytes", "ring_offset", "cur_len_offset", "pending_offset", "prefix_offset",
                                          "block_sum_offset")]
                + [(n, C.c_int32) for n in ("capacity", "num_envs", "row_floats", "pending_floats", "obs_dim",
                                            "goal_dim", "action_dim", "off_obs", "off_ag", "off_dg", "off_action",
                                            "off_next_obs", "off_next_ag", "off_reward", "off_terminated",
                                            "off_ep_end")])


class ReplayBatch(C.Structure):
    """ps_replay_batch: the outputs of a sample (device pointers; NULL skips one)."""
    _fields_ = [(n, C.c_void_p) for n in ("obs", "ag", "dg", "action", "next_obs", "next_ag", "reward", "terminated",
                                          "success", "relabelled", "env_idx", "slot", "goal_slot", "n_valid")]


class Layout(C.Structure):
    _fields_ = [
        ("num_envs", C.c_int64), ("stride", C.c_int64), ("float_offset", C.c_int64), ("goal_offset", C.c_int64),
        ("rng_offset", C.c_int64), ("elapsed_offset", C.c_int64), ("total_bytes", C.c_int64),
    ]


class PandasimError(RuntimeError):
    pass


_lib = None


V, I, I64, P = C.c_void_p, C.c_int, C.c_int64, C.POINTER
F, D = P(C.c_float), P(C.c_double)
# Every exported symbol (include/pandasim.h), once: name -> (argtypes, restype,
# group).  argtypes None leaves the ctypes default.  A group names symbols
# added within ABI version 6: a library built before them (one of the two that
# scripts/compare_libs.py loads under PANDASIM_LIB) still binds, and calling
# one on it raises AttributeError -- "oriented" the oriented step, "motion" the
# motion primitives (panda_cartesian.py move / grasp / release), "cloud" the
# fused point-cloud observation (PandaSim.point_cloud), "group" the PointNet++
# front end of that observation (PandaSim.group_cloud), "propagate" its
# feature propagation (PandaSim.propagate_features), "mlp" the shared MLP with
# max-pool (PandaSim.shared_mlp / abstract_features), "decode" the policy's
# waypoint decoding (PandaSim.decode_waypoints), "keypoint" the keypoint
# conditioning of the cloud's feature rows (PandaSim.keypoint_features),
# "bfloat" the shared MLP's learned layers in reduced precision (bfloat16 operands
# on the bf16 matrix cores: CloudMlp(..., precision="bfloat16")), "program" a
# whole sequence of motion primitives in one launch (PandaSim.motion_program),
# "replay" the device-resident HER replay buffer (pandasim.replay.HerReplay),
# "labels" the policy's demonstration labels and the forward value of its
# losses (PandaSim.label_cloud / policy_loss).
SIGNATURES = {
    "ps_abi_version": (None, I, None),
    "ps_default_config": ([I, I, I, P(Config)], I, None),
    "ps_state_layout": ([I64, P(Layout)], I, None),
    "ps_create": ([P(Config), I64, I, P(V)], I, None),
    "ps_destroy": ([V], None, None),
    "ps_last_error": ([V], C.c_char_p, None),
    "ps_obs_dim": ([V], I, None),
    "ps_action_dim": ([V], I, None),
    "ps_goal_dim": ([V], I, None),
    "ps_max_episode_steps": ([V], I, None),
    "ps_init_state": ([V, V, V], I, None),
    "ps_reset": ([V, V, V, V, V, V, V, V], I, None),
    "ps_step": ([V, V, V, V, V, V, V, V, V, I, V, V, V], I, None),
    "ps_sim_step": ([V, V, I, V], I, None),
    "ps_link_state": ([V, V, I, V, V, V, V, V], I, None),
    "ps_inverse_kinematics": ([V, V, I, V, V, V, V], I, None),
    "ps_compute_reward": ([I, I, V, I, V, I, V, V, I64, V], I, None),
    "ps_rng_seed": ([V, V, V, V, V], I, None),
    "ps_rng_uniform": ([V, V, V, I, D, D, V, V], I, None),
    "ps_rng_rotation": ([V, V, V, V, V], I, None),
    "ps_base_state": ([V, V, I, V, V, V, V, V, V], I, None),
    "ps_camera": ([F, C.c_float, C.c_float, C.c_float, C.c_float, I, I, F, F, D], I, None),
    "ps_render": ([V, V, F, F, I, I, P(Visual), V, V, V, V], I, None),
    "ps_deproject_image": ([V, V, D, I, I, V, V, V, V], I, None),
    "ps_deproject_pixels": ([V, V, V, I, D, I, I, V, V], I, None),
    "ps_set_nonfinite_guard": ([V, V, I], I, None),
    "ps_set_lanes_per_env": ([V, I], I, None),
    "ps_step_lanes": ([V], I, None),
    "ps_mark_motor_rows_dirty": ([V], I, None),
    "ps_set_episode_stats": ([V, V], I, None),
    "ps_step_oriented": ([V, V, V, V, V, V, V, V, V, V, I, V, V, V], I, "oriented"),
    "ps_euler_xyz_to_quat": ([V, V, V, I64, V], I, "oriented"),
    "ps_quat_to_euler_xyz": ([V, V, V, I64, V], I, "oriented"),
    "ps_motion_plan_bytes": ([I64], I64, "motion"),
    "ps_plan_move": ([V, V, V, V, V, V, V], I, "motion"),
    "ps_plan_grasp": ([V, V, V, V, V], I, "motion"),
    "ps_plan_release": ([V, V, V, V, V, V], I, "motion"),
    "ps_motion_run": ([V, V, V, I, V], I, "motion"),
    "ps_motion_program": ([V, V, V, I, P(C.c_int32), P(C.c_int32), I, V, V, V, V, V, V, V], I, "program"),
    "ps_cloud_workspace_bytes": ([I64, I, I, I], I64, "cloud"),
    "ps_point_cloud": ([V, V, V, I, I, I, P(Visual), V, V, I, C.c_uint64, V, V, V, V, V, V], I, "cloud"),
    "ps_cloud_normalize": ([V, V, I, V, V, V, V], I, "group"),
    "ps_cloud_fps": ([V, V, I, V, I, V, V], I, "group"),
    "ps_cloud_ball_query": ([V, V, I, V, I, C.c_double, I, V, V], I, "group"),
    "ps_cloud_group": ([V, V, V, I, I, V, I, V, I, V, V, V], I, "group"),
    "ps_cloud_set_abstraction": ([V, V, V, I, I, V, I, P(CloudScale), I, I, V, V, V, V, V, V], I, "group"),
    "ps_cloud_three_nn": ([V, V, I, V, I, V, V, V], I, "propagate"),
    "ps_cloud_interpolate": ([V, V, I, V, I, I, I, V, V, V, V], I, "propagate"),
    "ps_cloud_feature_propagation": ([V, V, I, V, I, V, I, V, I, V, V, V, V], I, "propagate"),
    "ps_cloud_mlp": ([V, V, I, I, P(CloudMlpLayer), I, I, V, I64, I, V], I, "mlp"),
    "ps_cloud_group_mlp": ([V, V, V, I, I, V, I, V, I, P(CloudMlpLayer), I, V, I64, I, V], I, "mlp"),
    "ps_cloud_mlp_bfloat": ([V, V, I, I, P(CloudMlpBfloatLayer), I, I, V, I64, I, V], I, "bfloat"),
    "ps_cloud_group_mlp_bfloat": ([V, V, V, I, I, V, I, V, I, P(CloudMlpBfloatLayer), I, V, I64, I, V], I, "bfloat"),
    "ps_cloud_decode_waypoints": ([V, V, I, I, I, V, V, V, C.c_uint32, C.c_uint32, V, V, V, V, V, V, V], I, "decode"),
    "ps_cloud_keypoint_features": ([V, V, P(CloudView), I, I, P(Visual), V, V, I, I, C.c_double, F, V, V, V, I, V, I, I, V,
                                    V], I, "keypoint"),
    "ps_cloud_waypoint_labels": ([V, V, V, V, V, V, V, C.c_double, V, I, V, V, I, I, V], I, "labels"),
    "ps_cloud_policy_loss": ([V, V, I, I, I, V, V, I, I, C.c_uint32, C.c_uint32, V, V, V, V], I, "labels"),
    "ps_replay_layout_of": ([V, I, P(ReplayLayout)], I, "replay"),
    "ps_replay_init": ([V, V, I, V], I, "replay"),
    "ps_replay_begin": ([V, V, I, I, I, V, V, V, V, V], I, "replay"),
    "ps_replay_store": ([V, V, I, I, V, V, V, V, V, V, V, V, V, V], I, "replay"),
    "ps_replay_sample": ([V, V, I, I, I, I, C.c_uint64, C.c_uint64, C.c_uint64, I64, P(ReplayBatch), V], I, "replay"),
}
ORIENTED_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "oriented")
MOTION_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "motion")
PROGRAM_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "program")
CLOUD_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "cloud")
GROUP_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "group")
PROPAGATE_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "propagate")
MLP_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "mlp")
BFLOAT_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "bfloat")
DECODE_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "decode")
KEYPOINT_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "keypoint")
REPLAY_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "replay")
LABELS_SYMBOLS = tuple(n for n, s in SIGNATURES.items() if s[2] == "labels")
REPLAY_FUTURE, REPLAY_FINAL = 0, 1
REPLAY_MAX_CAPACITY, REPLAY_MAX_ENVS, REPLAY_MAX_BATCH, REPLAY_SCAN_BLOCK = 1 << 20, 1 << 20, 1 << 27, 1024
CLOUD_MAX_VIEWS = 8
CLOUD_MAX_POINTS, CLOUD_MAX_SCALES, CLOUD_MAX_FEATURES = 8192, 4, 16
CLOUD_MAX_PROP_FEATURES, CLOUD_MAX_DENSE_POINTS = 2048, 1 << 20
CLOUD_MLP_MAX_LAYERS, CLOUD_MLP_MAX_HIDDEN, CLOUD_MLP_MAX_LAST = 4, 512, 1024
CLOUD_DECODE_MAX_CLASSES, CLOUD_DECODE_MAX_LD = 16, 4096
CLOUD_KEYPOINT_MAX, CLOUD_KEYPOINT_MAX_RADIUS, CLOUD_KEYPOINT_MAX_LD = 4, 8, 4096
CLOUD_LABEL_MAX_LD, CLOUD_LABEL_COLUMNS = 4096, 14


def exported_symbols():
    return list(SIGNATURES)



# the motion plan's rows (include/pandasim.h PS_PLAN_*): f64 rows, then i32 rows, of the state's stride
PLAN_START, PLAN_DELTA, PLAN_WIDTH, PLAN_Q0, PLAN_ROTVEC, PLAN_NUM_F64_ROWS = 0, 3, 6, 7, 11, 14
PLAN_NUM_STEPS, PLAN_DONE, PLAN_BLOCKED, PLAN_KIND, PLAN_NUM_I32_ROWS = 0, 1, 2, 3, 4
PLAN_KIND_MOVE, PLAN_KIND_HOLD, PLAN_HOLD_STEPS = 0, 1, 30
# the segments of a motion program (PS_SEG_*, PS_PROGRAM_*)
SEG_MOVE, SEG_GRASP, SEG_RELEASE, SEG_WAIT = 0, 1, 2, 3
PROGRAM_MAX_SEGMENTS, PROGRAM_MAX_WAIT = 32, 1000


def check_fresh(path: str) -> None:
    """Refuse a library built from other sources than the ones next to it
    (build.py's content stamp).  The product library and the named variants
    (libpandasim_<variant>.so) must carry a stamp equal to the sha256 of the
    current csrc/ and include/ files plus their flags; a library at any other
    path (an experiment under PANDASIM_LIB) is checked only if it has a stamp
    and its variant is known."""
    from . import build as B

    name = os.path.basename(path)
    variant = None
    if os.path.abspath(path) == os.path.abspath(B.OUT):
        variant = ""
    elif name.startswith("libpandasim_") and name.endswith(".so") and name[12:-3] in B.VARIANTS:
        variant = name[12:-3]
    if variant is None or not os.path.isdir(B.CSRC):
        return
    have = B.read_stamp(path)
    if have is None:
        if os.path.abspath(path) == os.path.abspath(B.OUT):
            raise PandasimError(f"{path} has no build stamp: rebuild it with `python -m pandasim.build`")
        return
    if have != B.fingerprint(variant):
        raise PandasimError(f"{path} is stale: its stamp does not match the sources in {B.CSRC} and "
                            f"{B.INCLUDE}; rebuild it with `python -m pandasim.build`")


def lib():
    """Load libpandasim.so (raises if it has not been built or is stale)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PandasimError(f"{LIB_PATH} not found: build it with `python -m pandasim.build` (hipcc, gfx950)")
    check_fresh(LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for name, (argtypes, restype, group) in SIGNATURES.items():
        if group and "PANDASIM_LIB" in os.environ and not hasattr(L, name):
            continue  # only a library named by PANDASIM_LIB may predate them
        fn = getattr(L, name)
        if argtypes is not None:
            fn.argtypes = argtypes
        fn.restype = restype
    _lib = L
    return L


def check(rc: int, ctx=None, what: str = "") -> None:
    if rc != PS_OK:
        msg = ""
        if ctx is not None:
            raw = lib().ps_last_error(ctx)
            msg = raw.decode() if raw else ""
        raise PandasimError(f"{what} failed: {ERRORS.get(rc, rc)} {msg}".strip())


def layout(num_envs: int) -> Layout:
    lay = Layout()
    check(lib().ps_state_layout(int(num_envs), C.byref(lay)), what="ps_state_layout")
    return lay


def default_config(task: int, control: int, reward: int) -> Config:
    cfg = Config()
    check(lib().ps_default_config(task, control, reward, C.byref(cfg)), what="ps_default_config")
    return cfg


def _ptr(t):
    """A tensor's address as a void-pointer argument; None stays NULL."""
    return None if t is None else C.c_void_p(t.data_ptr())
