"""ctypes binding of libray3d_hip.so (C ABI: include/ray3d_hip.h).

There is deliberately no fallback: if the shared library is missing or a call fails, this module
raises.  It never imports anything from ``oracle/``.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libray3d_hip.so")
# The hooks build (the same sources with -DR3D_TEST_HOOKS): the r3d_debug_* exports and the development switches read from
# the environment.  tests/ and tools/ select it with use_hooks(True); nothing in this package does.
# (R3D_HOOKS_LIB: another build of the hooks library, e.g. libray3d_hip_san.so - `make -C ray3d_amd/csrc san`: host objects under ASan / UBSan)
HOOKS_LIB_PATH = os.environ.get("R3D_HOOKS_LIB") or os.path.join(_HERE, "libray3d_hip_hooks.so")

R3D_KIND_POS, R3D_KIND_TRJ = 0, 1
R3D_INPUT_RAYS, R3D_INPUT_UV, R3D_INPUT_UV_DIST = 0, 1, 2
R3D_INPUT_PX_INTRINSIC, R3D_INPUT_PX_SCREEN = 3, 4     # the 2-feature models' inputs from raw pixels (same pre-pass kernel)
PX_MODES = (R3D_INPUT_UV_DIST, R3D_INPUT_PX_INTRINSIC, R3D_INPUT_PX_SCREEN)   # modes whose workspace carries the pre-pass's output
R3D_ERR_ARG, R3D_ERR_WORKSPACE = -1, -6
R3D_ERR_SHAPE, R3D_ERR_STATE = -3, -4
R3D_ERR_ABORTED = -7
R3D_OPT_STAGED, R3D_OPT_SPIN_TIMEOUT_MS, R3D_OPT_CU_LIMIT, R3D_OPT_LANES = 1, 2, 3, 4

# every symbol include/ray3d_hip.h declares (tests check the library exports exactly these)
EXPORTS = (
    "r3d_create", "r3d_destroy", "r3d_num_weights", "r3d_weight_key", "r3d_weight_shape",
    "r3d_set_weight", "r3d_finalize", "r3d_workspace_bytes", "r3d_forward", "r3d_forward_pair",
    "r3d_profile_enable", "r3d_profile_read", "r3d_clip_metrics", "r3d_clip_metrics_detail", "r3d_clip_valid_losses", "r3d_last_error", "r3d_version",
    "r3d_prepare", "r3d_release", "r3d_abi_version", "r3d_precision", "r3d_status", "r3d_set_option", "r3d_last_clock",
    "r3d_lane_stream", "r3d_lanes_join", "r3d_input_workspace_bytes", "r3d_clips_metrics", "r3d_clips_metrics_scratch_bytes",
    "r3d_clips_encode", "r3d_clips_valid_losses", "r3d_clips_valid_scratch_bytes", "r3d_clips_poses",
    "r3d_clips_project", "r3d_forward_pair_split", "r3d_finalize_dev", "r3d_clips_windows",
    "r3d_streams_state_bytes", "r3d_streams_step", "r3d_streams_poses", "r3d_streams_track_bytes", "r3d_streams_repair",
    "r3d_streams_peek", "r3d_streams_fuse", "r3d_streams_assign_bytes", "r3d_streams_assign", "r3d_streams_link_bytes",
    "r3d_streams_link", "r3d_clips_repair",
)
HOOK_EXPORTS = ("r3d_debug_schedule_check", "r3d_debug_plan_check", "r3d_debug_forward_check",   # libray3d_hip_hooks.so only
                "r3d_debug_forward_census", "r3d_debug_census_domain", "r3d_debug_plan_kind_edges",
                "r3d_debug_undistort_host", "r3d_debug_encode_px_host", "r3d_debug_valid_losses_host",
                "r3d_debug_clips_encode_host", "r3d_debug_clips_valid_losses_host", "r3d_debug_clips_poses_host",
                "r3d_debug_clips_project_host", "r3d_debug_pack_replay_host", "r3d_debug_weights_image",
                "r3d_debug_clips_windows_host", "r3d_debug_streams_step_host", "r3d_debug_streams_poses_host",
                "r3d_debug_streams_repair_host", "r3d_debug_streams_peek_host", "r3d_debug_streams_fuse_host",
                "r3d_debug_streams_assign_host", "r3d_debug_streams_link_host", "r3d_debug_plan_buffers", "r3d_debug_call_check",
                "r3d_debug_clips_repair_host")
ABI_VERSION = 6                                                          # R3D_ABI_VERSION of the header this binding follows
METRIC_NAMES = ("mpjpe", "p_mpjpe", "n_mpjpe", "velocity", "root")     # R3D_METRIC_* order
METRIC_OUT_DOUBLES = 5 * (1 + 128)                                      # R3D_METRIC_OUT_DOUBLES
DETAIL_THRESHOLDS, DETAIL_JOINT_ROWS, DETAIL_MAX_JOINTS = 31, 3, 17    # R3D_DETAIL_THRESHOLDS, _JOINT_ROWS, joint-row width
DETAIL_DOUBLES = DETAIL_JOINT_ROWS * DETAIL_MAX_JOINTS + DETAIL_THRESHOLDS   # R3D_DETAIL_DOUBLES (82)
DETAIL_OUT_DOUBLES = DETAIL_DOUBLES * (1 + 128)                         # R3D_DETAIL_OUT_DOUBLES
R3D_VALID_POS_IS_SUM, R3D_VALID_GT_ROOT_RELATIVE = 1, 2                 # flags of r3d_clip_valid_losses
VALID_NAMES = ("loss", "pos", "trj_w", "trj_wsum", "trj_dsum", "bone_len", "bone_dir")   # R3D_VALID_* order
VALID_COUNT, VALID_MAX_BONES, VALID_BONE_ROWS = 7, 16, 4                # R3D_VALID_COUNT, _MAX_BONES, _BONE_ROWS
VALID_DOUBLES = VALID_COUNT + VALID_BONE_ROWS * VALID_MAX_BONES         # R3D_VALID_DOUBLES (71)
VALID_OUT_DOUBLES = VALID_DOUBLES * (1 + 128)                           # R3D_VALID_OUT_DOUBLES
METRIC_COUNT, METRIC_MAX_BLOCKS, METRIC_THREADS = 5, 128, 256           # R3D_METRIC_COUNT, _MAX_BLOCKS; frames per workgroup
CLIPS_MAX = 65535                                                       # R3D_CLIPS_MAX
R3D_ENCODE_RAY, R3D_ENCODE_INTRINSIC, R3D_ENCODE_SCREEN = 0, 1, 2       # `encoding` of r3d_clips_encode
ENCODE_FLOATS = {R3D_ENCODE_RAY: 3, R3D_ENCODE_INTRINSIC: 2, R3D_ENCODE_SCREEN: 2}   # floats per encoded keypoint
ENCODE_MAX_POINTS = 2 ** 31 - 257                                       # R3D_ENCODE_MAX_POINTS
CLIP_INPUT_DESC_BYTES = 160                                             # sizeof(r3d_clip_input_desc)
REPAIR_MAX_ROWS = 65536                                                 # R3D_REPAIR_MAX_ROWS
REPAIR_STATE_NAMES = ("observed", "interpolated", "held", "back_filled", "never_observed")   # `state` of r3d_clips_repair, 0..4


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("struct_size", "kind", "num_joints", "in_features", "num_levels",
                                         "channels", "latent", "stage", "extrinsic_dim",
                                         "embed_dim", "causal", "dense", "bf16x3")]


class Input(C.Structure):
    _fields_ = [("mode", C.c_int32), ("x_dev", C.c_void_p), ("window_stride", C.c_int64),
                ("param_dev", C.c_void_p), ("param_stride", C.c_int64),
                ("cam_dev", C.c_void_p), ("cam_stride", C.c_int64)]


class ClipDesc(C.Structure):
    """r3d_clip_desc: one row of the device-side table r3d_clips_metrics reads (112 bytes)."""
    _fields_ = [("first_frame", C.c_int64), ("n_frames", C.c_int64), ("rn2w", C.c_double * 9), ("tn2w", C.c_double * 3)]


def clip_desc_dtype():
    """The NumPy structured dtype with r3d_clip_desc's layout: an array of it, uploaded as bytes, is the table."""
    import numpy as np
    return np.dtype([("first_frame", np.int64), ("n_frames", np.int64), ("rn2w", np.float64, (9,)), ("tn2w", np.float64, (3,))])


CLIP_DESC_BYTES = clip_desc_dtype().itemsize                            # sizeof(r3d_clip_desc)


def clip_input_desc_dtype():
    """The NumPy structured dtype with r3d_clip_input_desc's layout (160 bytes): an array of it, uploaded as bytes, is the
    table r3d_clips_encode reads."""
    import numpy as np
    return np.dtype([("first_frame", np.int64), ("n_frames", np.int64), ("out_first", np.int64),
                     ("pad_front", np.int32), ("pad_back", np.int32), ("cam", np.float64, (16,))])


def clip_project_desc_dtype():
    """The NumPy structured dtype with r3d_clip_project_desc's layout (360 bytes): an array of it, uploaded as bytes, is the
    table r3d_clips_project reads."""
    import numpy as np
    return np.dtype([("first_frame", np.int64), ("n_frames", np.int64), ("out_first", np.int64), ("gt_first", np.int64),
                     ("pad_front", np.int32), ("pad_back", np.int32), ("proj", np.float64, (12,)), ("cam", np.float64, (16,)),
                     ("rw2g", np.float64, (9,)), ("tw2g", np.float64, (3,))])


CLIP_PROJECT_DESC_BYTES = 360                                           # sizeof(r3d_clip_project_desc)


def window_run_dtype():
    """The NumPy structured dtype with r3d_window_run_desc's layout (48 bytes): an array of it, uploaded as bytes, is the table
    r3d_clips_windows reads."""
    import numpy as np
    return np.dtype([("first_frame", np.int64), ("n_frames", np.int64), ("win_first", np.int64), ("n_windows", np.int64),
                     ("start", np.int64), ("step", np.int32), ("flip", np.int32)])


WINDOW_RUN_DESC_BYTES = 48                                              # sizeof(r3d_window_run_desc)
R3D_ENCODE_NONE = 3                                                     # r3d_streams_step only: model-input rows, copied bit for bit
R3D_STREAM_IDLE, R3D_STREAM_PUSH, R3D_STREAM_RESTART, R3D_STREAM_DRAIN = 0, 1, 2, 3   # action words of r3d_streams_step
STREAMS_PEEK_MAX = 8                                                    # R3D_STREAMS_PEEK_MAX: looks per r3d_streams_peek call
FUSE_MAX_MEMBERS = 16                                                   # R3D_FUSE_MAX_MEMBERS: slots per group of r3d_streams_fuse
ASSIGN_MAX_SLOTS, ASSIGN_MAX_DETECTIONS = 32, 32                        # R3D_ASSIGN_MAX_SLOTS, R3D_ASSIGN_MAX_DETECTIONS
LINK_MAX_PEOPLE = 32                                                    # R3D_LINK_MAX_PEOPLE: people per scene of r3d_streams_link
R3D_ASSIGN_FILL_NAN, R3D_ASSIGN_FILL_HOLD = 0, 1                        # what an unmatched live slot of r3d_streams_assign pushes
STREAM_HEAD_BYTES = 16                                                  # sizeof(r3d_stream_head)


def stream_head_dtype():
    """The NumPy structured dtype with r3d_stream_head's layout (16 bytes): the front of a r3d_streams_step state viewed as an array
    of it is the streams' heads."""
    import numpy as np
    return np.dtype([("count", np.int64), ("drained", np.int64)])


def stream_pose_desc_dtype():
    """The NumPy structured dtype with r3d_stream_pose_desc's layout (112 bytes): an array of it, uploaded as bytes, is the table
    r3d_streams_poses reads - a (S, 14) float64 array of :meth:`Camera.stream_pose_row` rows has the same bytes."""
    import numpy as np
    return np.dtype([("rn2w", np.float64, (9,)), ("tn2w", np.float64, (3,)), ("height", np.float64), ("reserved", np.float64)])


STREAM_POSE_DESC_BYTES = 112                                            # sizeof(r3d_stream_pose_desc)

WINDOWS_BATCH_MAX = 65535                                               # `batch` of r3d_clips_windows (the grid's second dimension)


class LaunchRecord(C.Structure):
    _fields_ = [("kernel", C.c_char * 48), ("stage", C.c_int32), ("blocks", C.c_int32),
                ("ms", C.c_float), ("flops", C.c_double), ("bytes", C.c_double)]


class CensusRow(C.Structure):
    """r3d_census_row: one (launch, tile kind) of r3d_debug_forward_census."""
    _fields_ = [("launch", C.c_int32), ("blocks", C.c_int32), ("tiles", C.c_int32), ("kernel", C.c_char * 48),
                ("tile_kind", C.c_char * 48)]


class PlanBufferRow(C.Structure):
    """r3d_plan_buffer_row: one workspace buffer of r3d_debug_plan_buffers."""
    _fields_ = [("name", C.c_char * 48), ("floats_per_window", C.c_int64), ("offset_bytes", C.c_uint64), ("bytes", C.c_uint64),
                ("per_frame", C.c_int32), ("reserved", C.c_int32)]


class Ray3DHipError(RuntimeError):
    pass


_libs = {}
_hooks = os.environ.get("R3D_USE_HOOKS_LIB", "0") not in ("", "0")   # (tools/: A/B runs of bench.py on the hooks build)


_live = {}      # library path -> number of live Handles it created


def use_hooks(on: bool) -> None:
    """Tests / tools: make load() return libray3d_hip_hooks.so (True) or the product library (False, the default).  Handles
    belong to the library that created them: switch before building modules, and do not carry them across a switch.
    The two libraries are two copies of the same code with their OWN process-wide state - in particular the ordering of
    single-launch forwards of different streams (each needs every CU): forwards issued through both copies are not ordered
    against each other.  So when handles of the library being left are still alive, the switch first waits for the device -
    nothing of theirs is in flight when the other copy launches.  Do not run forwards of both copies concurrently."""
    global _hooks
    if bool(on) != _hooks and _live.get(HOOKS_LIB_PATH if _hooks else LIB_PATH, 0) > 0:
        try:
            import torch
            if torch.cuda.is_available():
                torch.cuda.synchronize()
        except ImportError:
            pass
    _hooks = bool(on)


def load():
    """Load libray3d_hip.so (or, after use_hooks(True), its hooks build); raise (never fall back) when it is not there."""
    path = HOOKS_LIB_PATH if _hooks else LIB_PATH
    if path in _libs:
        return _libs[path]
    if not os.path.exists(path):
        raise Ray3DHipError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % path)
    lib = C.CDLL(path)
    vp, i64p = C.c_void_p, C.POINTER(C.c_int64)
    lib.r3d_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    lib.r3d_destroy.argtypes = [vp]
    lib.r3d_num_weights.argtypes = [vp]
    lib.r3d_weight_key.argtypes = [vp, C.c_int]
    lib.r3d_weight_key.restype = C.c_char_p
    lib.r3d_weight_shape.argtypes = [vp, C.c_int, i64p, C.POINTER(C.c_int)]
    lib.r3d_set_weight.argtypes = [vp, C.c_char_p, vp, i64p, C.c_int]
    lib.r3d_finalize.argtypes = [vp]
    lib.r3d_finalize_dev.argtypes = [vp, C.POINTER(vp), i64p, C.c_int32, vp]
    lib.r3d_workspace_bytes.argtypes = [vp, vp, C.c_int64]
    lib.r3d_workspace_bytes.restype = C.c_size_t
    lib.r3d_input_workspace_bytes.argtypes = [vp, vp, C.POINTER(Input), C.c_int64]
    lib.r3d_input_workspace_bytes.restype = C.c_size_t
    lib.r3d_forward.argtypes = [vp, C.POINTER(Input), C.c_int64, vp, vp, C.c_size_t, vp]
    lib.r3d_forward_pair.argtypes = [vp, vp, C.POINTER(Input), C.c_int64, vp, vp, vp, C.c_size_t, vp]
    lib.r3d_forward_pair_split.argtypes = [vp, vp, C.POINTER(Input), C.c_int64, vp, vp, vp, C.c_size_t, vp]
    lib.r3d_prepare.argtypes = [vp, vp, C.c_int64]
    lib.r3d_release.argtypes = [vp, vp, C.c_int64]
    lib.r3d_precision.argtypes = [vp]
    lib.r3d_status.argtypes = [vp, vp]
    lib.r3d_set_option.argtypes = [vp, C.c_int32, C.c_int64]
    lib.r3d_last_clock.argtypes = [vp, vp, C.POINTER(C.c_double)]
    lib.r3d_lane_stream.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    lib.r3d_lanes_join.argtypes = [vp, vp]
    lib.r3d_profile_enable.argtypes = [vp, C.c_int]
    lib.r3d_profile_read.argtypes = [vp, C.POINTER(LaunchRecord), C.c_int]
    lib.r3d_clip_metrics.argtypes = [vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, vp]
    lib.r3d_clip_metrics_detail.argtypes = [vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_double), vp, vp, vp, vp]
    lib.r3d_clip_valid_losses.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, vp, vp, vp]
    lib.r3d_clips_metrics_scratch_bytes.argtypes = [C.c_int32, C.c_int64, C.c_int]
    lib.r3d_clips_metrics_scratch_bytes.restype = C.c_size_t
    lib.r3d_clips_metrics.argtypes = [vp, vp, C.c_int64, C.c_int32, vp, C.c_int32, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, vp, C.c_size_t, vp]
    lib.r3d_clips_encode.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int64, vp, C.c_int64, vp,
                                     C.POINTER(C.c_int32), vp, vp]
    lib.r3d_clips_repair.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, vp, C.POINTER(C.c_int32), vp, C.c_int32, C.c_int64, vp, C.c_int64,
                                     C.c_float, C.c_int32, vp, vp, vp, vp]
    lib.r3d_clips_valid_scratch_bytes.argtypes = [C.c_int32, C.c_int64]
    lib.r3d_clips_valid_scratch_bytes.restype = C.c_size_t
    lib.r3d_clips_valid_losses.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, vp, C.c_int32, C.c_int64,
                                           vp, C.c_int64, vp, vp, C.c_size_t, vp]
    lib.r3d_clips_poses.argtypes = [vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_int32), vp, vp, C.c_int32, C.c_int64, vp, vp, C.c_int64,
                                    vp, vp]
    lib.r3d_clips_project.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int64, vp, C.c_int64, vp,
                                      C.POINTER(C.c_int32), vp, vp, C.c_int64, vp, vp, vp]
    lib.r3d_clips_windows.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_int32, C.c_int64, C.c_int64,
                                      vp, vp, C.POINTER(C.c_int32), vp, vp]
    lib.r3d_streams_state_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.r3d_streams_state_bytes.restype = C.c_size_t
    lib.r3d_streams_step.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp,
                                     C.POINTER(C.c_int32), vp, vp, vp]
    lib.r3d_streams_poses.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), vp, vp, vp, vp, vp, C.c_int32, C.c_int32,
                                      vp, vp, vp, vp, vp]
    lib.r3d_streams_track_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.r3d_streams_track_bytes.restype = C.c_size_t
    lib.r3d_streams_repair.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, C.c_float, vp, vp,
                                       C.c_int32, vp, vp, vp]
    lib.r3d_streams_peek.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, vp, vp, vp,
                                     vp, C.POINTER(C.c_int32), vp, vp, vp]
    lib.r3d_streams_fuse.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double,
                                     vp, vp, vp, vp, vp]
    lib.r3d_streams_assign_bytes.restype = C.c_size_t
    lib.r3d_streams_assign_bytes.argtypes = [C.c_int32] * 4
    lib.r3d_streams_assign.argtypes = [vp] * 12
    lib.r3d_streams_link_bytes.restype = C.c_size_t
    lib.r3d_streams_link_bytes.argtypes = [C.c_int32] * 4
    lib.r3d_streams_link.argtypes = [vp] * 11
    lib.r3d_last_error.restype = C.c_char_p
    lib.r3d_version.restype = C.c_char_p
    if _hooks:
        lib.r3d_debug_clips_repair_host.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, vp, C.POINTER(C.c_int32), vp, C.c_int32, C.c_int64, vp,
                                                    C.c_int64, C.c_float, C.c_int32, vp, vp, vp]
        lib.r3d_debug_streams_assign_host.argtypes = [vp] * 11
        lib.r3d_debug_streams_link_host.argtypes = [vp] * 10
        lib.r3d_debug_streams_fuse_host.argtypes = [vp, vp, vp, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int32, C.c_double, C.c_double,
                                                    C.c_double, vp, vp, vp, vp]
        lib.r3d_debug_streams_peek_host.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32),
                                                    C.c_int32, vp, vp, vp, vp, C.POINTER(C.c_int32), vp, vp]
        lib.r3d_debug_streams_repair_host.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp,
                                                      C.c_float, vp, vp, C.c_int32, vp, vp]
        lib.r3d_debug_streams_poses_host.argtypes = [vp, vp, C.c_int32, C.c_int32, C.POINTER(C.c_int32), vp, vp, vp, vp, vp, C.c_int32,
                                                     C.c_int32, vp, vp, vp, vp]
        lib.r3d_debug_streams_step_host.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp,
                                                    C.POINTER(C.c_int32), vp, vp]
        lib.r3d_debug_clips_windows_host.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_int32, C.c_int64,
                                                     C.c_int64, vp, vp, C.POINTER(C.c_int32), vp]
        lib.r3d_debug_pack_replay_host.argtypes = [vp, i64p, i64p]
        lib.r3d_debug_weights_image.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.r3d_debug_clips_project_host.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int64, vp, C.c_int64, vp,
                                                     C.POINTER(C.c_int32), vp, vp, C.c_int64, vp, vp]
        lib.r3d_debug_forward_census.argtypes = [vp, vp, C.c_int64, C.c_int, C.c_int32, C.c_int64, C.c_int64, C.c_int32, C.c_int32,
                                                 C.POINTER(CensusRow), C.c_int32]
        lib.r3d_debug_census_domain.argtypes = [C.POINTER(CensusRow), C.c_int32]
        lib.r3d_debug_plan_kind_edges.argtypes = [i64p, C.c_int32]
        lib.r3d_debug_plan_buffers.argtypes = [vp, vp, C.c_int64, C.POINTER(PlanBufferRow), C.c_int32, C.POINTER(C.c_uint64)]
        lib.r3d_debug_call_check.argtypes = [vp, vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int32)]
        lib.r3d_debug_clips_poses_host.argtypes = [vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_int32), vp, vp, C.c_int32, C.c_int64, vp, vp,
                                                   C.c_int64, vp]
        lib.r3d_debug_clips_valid_losses_host.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, vp, C.c_int32,
                                                          C.c_int64, vp, C.c_int64, vp]
        lib.r3d_debug_undistort_host.argtypes = [vp, vp, C.c_int64, vp, vp]
        lib.r3d_debug_encode_px_host.argtypes = [vp, vp, C.c_int64, C.c_int32, vp]
        lib.r3d_debug_valid_losses_host.argtypes = [vp, vp, vp, C.c_int64, C.c_int32, C.POINTER(C.c_int32), C.c_int32, vp, vp]
        lib.r3d_debug_clips_encode_host.argtypes = [vp, C.c_int64, C.c_int32, C.c_int32, vp, C.c_int32, C.c_int64, vp, C.c_int64, vp,
                                                    C.POINTER(C.c_int32), vp]
    for name in EXPORTS + (HOOK_EXPORTS if _hooks else ()):
        fn = getattr(lib, name)
        if fn.restype is C.c_int or fn.restype is None:
            fn.restype = C.c_int
    if lib.r3d_abi_version() != ABI_VERSION:
        raise Ray3DHipError("%s has ABI version %d, this binding was written for %d: rebuild the library"
                            % (path, lib.r3d_abi_version(), ABI_VERSION))
    _libs[path] = lib
    return lib


def check(rc: int, what: str):
    if rc < 0:
        raise Ray3DHipError("%s failed (%d): %s" % (what, rc, load().r3d_last_error().decode()))
    return rc


class Handle:
    """Owns one r3d_model*."""

    def __init__(self, cfg):
        lib = self._lib = load()          # (a handle stays with the library that created it: see use_hooks)
        self.options = {}                 # R3D_OPT_* -> the value last set through set_option
        c = Config(C.sizeof(Config), R3D_KIND_POS if cfg.kind == "pos" else R3D_KIND_TRJ, cfg.num_joints,
                   cfg.in_features, len(cfg.filter_widths), cfg.channels, cfg.latent, cfg.stage,
                   cfg.extrinsic_dim if cfg.camera_embedding else 0,
                   cfg.embed_dim if cfg.camera_embedding else 0, 1 if cfg.causal else 0,
                   1 if cfg.dense_convs else 0, 1 if getattr(cfg, "bf16x3", False) else 0)
        self.ptr = C.c_void_p()
        check(lib.r3d_create(C.byref(c), C.byref(self.ptr)), "r3d_create")
        self._lib_path = HOOKS_LIB_PATH if lib is _libs.get(HOOKS_LIB_PATH) else LIB_PATH
        _live[self._lib_path] = _live.get(self._lib_path, 0) + 1

    def keys(self) -> List[str]:
        lib = self._lib
        return [lib.r3d_weight_key(self.ptr, i).decode() for i in range(lib.r3d_num_weights(self.ptr))]

    def shape(self, index: int):
        shp = (C.c_int64 * 4)()
        rank = C.c_int()
        check(self._lib.r3d_weight_shape(self.ptr, index, shp, C.byref(rank)), "r3d_weight_shape")
        return tuple(int(shp[i]) for i in range(rank.value))

    def set_weight(self, key: str, array):
        """array: C-contiguous float32 numpy array in torch layout."""
        shp = (C.c_int64 * 4)(*([int(d) for d in array.shape] + [1] * (4 - array.ndim)))
        check(self._lib.r3d_set_weight(self.ptr, key.encode(), array.ctypes.data_as(C.c_void_p), shp,
                                    array.ndim), "r3d_set_weight(%s)" % key)

    def finalize(self):
        check(self._lib.r3d_finalize(self.ptr), "r3d_finalize")

    def finalize_dev_raw(self, ptrs, numel, count: int, stream: int) -> int:
        """r3d_finalize_dev as the C ABI takes it (`ptrs` / `numel`: ctypes arrays or None); returns the status code."""
        return int(self._lib.r3d_finalize_dev(self.ptr, ptrs, numel, count, stream))

    def finalize_dev(self, tensors, stream: int):
        """r3d_finalize_dev: `tensors` one contiguous float32 device tensor per key of :meth:`keys`, in that order (anything with
        data_ptr() and numel()); the pack is ordered on `stream`.  The tensors must stay alive until the stream has passed it."""
        n = len(tensors)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in tensors])
        numel = (C.c_int64 * n)(*[int(t.numel()) for t in tensors])
        check(self.finalize_dev_raw(ptrs, numel, n, stream), "r3d_finalize_dev")

    def debug_pack_replay_host(self):
        """r3d_debug_pack_replay_host (hooks library only): ``(mismatches, first_index)`` of the device path's tables and routines
        replayed on the CPU against the host pack of the weights set so far."""
        mism, first = C.c_int64(-1), C.c_int64(-1)
        check(self._lib.r3d_debug_pack_replay_host(self.ptr, C.byref(mism), C.byref(first)), "r3d_debug_pack_replay_host")
        return int(mism.value), int(first.value)

    def debug_weights_image(self):
        """r3d_debug_weights_image (hooks library only): the packed image on the device as a float32 numpy array."""
        import numpy as np
        need = C.c_size_t(0)
        rc = self._lib.r3d_debug_weights_image(self.ptr, None, 0, C.byref(need))
        if rc != R3D_ERR_WORKSPACE:
            check(rc, "r3d_debug_weights_image")
        out = np.empty(int(need.value), np.float32)
        check(self._lib.r3d_debug_weights_image(self.ptr, out.ctypes.data_as(C.c_void_p), out.size, C.byref(need)), "r3d_debug_weights_image")
        return out

    def precision(self) -> str:
        """'f32' or 'bf16x3': what the handle's large GEMMs run in (r3d_config.bf16x3 or the R3D_BF16X3 override)."""
        return "bf16x3" if check(self._lib.r3d_precision(self.ptr), "r3d_precision") == 1 else "f32"

    def set_option(self, option: int, value: int):
        check(self._lib.r3d_set_option(self.ptr, option, value), "r3d_set_option")
        self.options[int(option)] = int(value)

    def lane_stream(self, lane: int) -> int:
        """r3d_lane_stream: the hipStream_t of lane `lane` of a handle with R3D_OPT_LANES (the library owns it)."""
        st = C.c_void_p()
        check(self._lib.r3d_lane_stream(self.ptr, lane, C.byref(st)), "r3d_lane_stream")
        return int(st.value)

    def lanes_join(self, stream: int):
        """r3d_lanes_join: `stream` waits for the forwards the library relayed to lanes from other streams."""
        check(self._lib.r3d_lanes_join(self.ptr, stream), "r3d_lanes_join")

    def status(self, stream: int) -> bool:
        """r3d_status: synchronises `stream`; True when every forward of this handle since the last call finished, False
        when one gave up waiting for its own tiles (outputs NaN; the flag is cleared)."""
        rc = self._lib.r3d_status(self.ptr, stream)
        if rc == R3D_ERR_ABORTED:
            return False
        check(rc, "r3d_status")
        return True

    def last_clock_ghz(self, stream: int) -> float:
        """r3d_last_clock: the shader clock the handle's last single-launch forward ran at (0.0: none / level by level)."""
        ghz = C.c_double(0.0)
        check(self._lib.r3d_last_clock(self.ptr, stream, C.byref(ghz)), "r3d_last_clock")
        return float(ghz.value)

    def profile_enable(self, on: bool):
        check(self._lib.r3d_profile_enable(self.ptr, 1 if on else 0), "r3d_profile_enable")

    def profile_read(self):
        cap = 128
        recs = (LaunchRecord * cap)()
        n = check(self._lib.r3d_profile_read(self.ptr, recs, cap), "r3d_profile_read")
        return [dict(kernel=recs[i].kernel.decode(), stage=recs[i].stage, blocks=recs[i].blocks,
                     ms=recs[i].ms, flops=recs[i].flops, bytes=recs[i].bytes) for i in range(min(n, cap))]

    def close(self):
        if getattr(self, "ptr", None) and self.ptr.value and getattr(self, "_lib", None) is not None:
            self._lib.r3d_destroy(self.ptr)
            self.ptr = C.c_void_p()
            _live[self._lib_path] = _live.get(self._lib_path, 1) - 1

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _lib_of(*handles):
    """The library the given handles belong to (the selected one when there is none)."""
    for h in handles:
        if h is not None:
            return h._lib
    return load()


def workspace_bytes(pos: Optional[Handle], trj: Optional[Handle], batch: int) -> int:
    return int(_lib_of(pos, trj).r3d_workspace_bytes(pos.ptr if pos else None, trj.ptr if trj else None, batch))


def input_workspace_bytes(pos: Optional[Handle], trj: Optional[Handle], inp: Input, batch: int) -> int:
    """r3d_input_workspace_bytes: the workspace of forwards of at most `batch` windows with inputs shaped as `inp` (for
    R3D_INPUT_UV_DIST: r3d_workspace_bytes + the pre-pass's ray buffer; for R3D_INPUT_PX_INTRINSIC / _SCREEN the same with 2
    floats per point).  Raises on bad arguments (the library returns 0)."""
    n = int(_lib_of(pos, trj).r3d_input_workspace_bytes(pos.ptr if pos else None, trj.ptr if trj else None, C.byref(inp), batch))
    if n == 0:
        raise Ray3DHipError("r3d_input_workspace_bytes failed: %s" % _lib_of(pos, trj).r3d_last_error().decode())
    return n


def prepare(pos: Optional[Handle], trj: Optional[Handle], batch: int):
    """r3d_prepare: plan + tile schedule of this batch size, uploaded (outside of any stream capture)."""
    check(_lib_of(pos, trj).r3d_prepare(pos.ptr if pos else None, trj.ptr if trj else None, batch), "r3d_prepare")


def release(pos: Optional[Handle], trj: Optional[Handle], batch: int):
    """r3d_release: un-pin a batch size named in prepare() (after the hipGraph that captured it is gone)."""
    check(_lib_of(pos, trj).r3d_release(pos.ptr if pos else None, trj.ptr if trj else None, batch), "r3d_release")


def make_input(mode, x_ptr, window_stride, param_ptr, param_stride, cam_ptr=None, cam_stride=0) -> Input:
    return Input(mode, x_ptr, window_stride, param_ptr, param_stride, cam_ptr, cam_stride)


def forward(handle: Handle, inp: Input, batch: int, out_ptr: int, ws_ptr: int, ws_bytes: int, stream: int):
    check(handle._lib.r3d_forward(handle.ptr, C.byref(inp), batch, out_ptr, ws_ptr, ws_bytes, stream),
          "r3d_forward")


def clip_metrics(pred_ptr: int, gt_ptr: int, n_frames: int, num_joints: int, rn2w, tn2w, out_ptr: int, stream: int):
    """r3d_clip_metrics: rn2w (3,3) / tn2w (3,) float64 array-likes on the host; the rest device pointers."""
    r = (C.c_double * 9)(*[float(v) for row in rn2w for v in row])
    t = (C.c_double * 3)(*[float(v) for v in tn2w])
    check(load().r3d_clip_metrics(pred_ptr, gt_ptr, n_frames, num_joints, r, t, out_ptr, stream), "r3d_clip_metrics")


def clip_metrics_detail(pred_ptr: int, gt_ptr: int, n_frames: int, num_joints: int, rn2w, tn2w, out_ptr: int,
                        frame_ptr: Optional[int], detail_ptr: int, stream: int):
    """r3d_clip_metrics_detail: clip_metrics plus `frame_ptr` ((n_frames, 5) float64 device memory, or None) and
    `detail_ptr` (DETAIL_OUT_DOUBLES float64, the first DETAIL_DOUBLES are the results)."""
    r = (C.c_double * 9)(*[float(v) for row in rn2w for v in row])
    t = (C.c_double * 3)(*[float(v) for v in tn2w])
    check(load().r3d_clip_metrics_detail(pred_ptr, gt_ptr, n_frames, num_joints, r, t, out_ptr, frame_ptr or None, detail_ptr,
                                         stream), "r3d_clip_metrics_detail")


def clips_metrics_scratch_bytes(num_clips: int, max_frames: int, detail: bool) -> int:
    """r3d_clips_metrics_scratch_bytes: the scratch one r3d_clips_metrics call over `num_clips` clips of at most `max_frames`
    frames needs (0 for num_clips < 1 or max_frames < 1)."""
    return int(load().r3d_clips_metrics_scratch_bytes(num_clips, max_frames, 1 if detail else 0))


def clips_metrics(pred_ptr: int, gt_ptr: int, total_frames: int, num_joints: int, table_ptr: int, num_clips: int, max_frames: int,
                  rows_ptr: int, row_stride: int, detail_ptr: Optional[int], detail_stride: int, frame_ptr: Optional[int],
                  scratch_ptr: int, scratch_bytes: int, stream: int):
    """r3d_clips_metrics: every pointer is device memory; `table_ptr` num_clips r3d_clip_desc (:func:`clip_desc_dtype`) back to
    back; `detail_ptr` / `frame_ptr` may be None."""
    check(load().r3d_clips_metrics(pred_ptr, gt_ptr, total_frames, num_joints, table_ptr, num_clips, max_frames, rows_ptr, row_stride,
                                   detail_ptr or None, detail_stride, frame_ptr or None, scratch_ptr, scratch_bytes, stream),
          "r3d_clips_metrics")


def clips_encode(px_ptr: int, total_frames: int, num_joints: int, encoding: int, table_ptr: int, num_clips: int, max_rows: int,
                 x_ptr: int, out_rows: int, x_mirror_ptr: Optional[int], mirror_perm, status_ptr: int, stream: int):
    """r3d_clips_encode: every pointer is device memory; `table_ptr` num_clips r3d_clip_input_desc
    (:func:`clip_input_desc_dtype`) back to back; `x_mirror_ptr` (or None) and `mirror_perm` (a host sequence of num_joints
    ints, or None) go together; `status_ptr` num_clips int32."""
    if mirror_perm is not None and len(mirror_perm) != num_joints:
        raise Ray3DHipError("r3d_clips_encode: mirror_perm has %d entries, num_joints is %d" % (len(mirror_perm), num_joints))
    perm = (C.c_int32 * len(mirror_perm))(*[int(v) for v in mirror_perm]) if mirror_perm is not None else None
    check(load().r3d_clips_encode(px_ptr, total_frames, num_joints, encoding, table_ptr, num_clips, max_rows, x_ptr, out_rows,
                                  x_mirror_ptr or None, perm, status_ptr, stream), "r3d_clips_encode")


def _mirror_table(what: str, mirror_perm, num_joints: int):
    if mirror_perm is None:
        return None
    if len(mirror_perm) != num_joints:
        raise Ray3DHipError("%s: mirror_perm has %d entries, num_joints is %d" % (what, len(mirror_perm), num_joints))
    return (C.c_int32 * len(mirror_perm))(*[int(v) for v in mirror_perm])


def clips_repair(x_ptr: int, out_rows: int, num_joints: int, in_features: int, x_mirror_ptr: Optional[int], mirror_perm, table_ptr: int,
                 num_clips: int, max_rows: int, conf_ptr: Optional[int], total_frames: int, min_conf: float, max_gap: int,
                 state_ptr: Optional[int], stats_ptr: Optional[int], status_ptr: int, stream: int):
    """r3d_clips_repair (enqueued BEHIND :func:`clips_encode`, with its table, `out_rows` and `max_rows`): every pointer is device
    memory; `x_ptr` (out_rows, num_joints, in_features) float32, repaired in place; `x_mirror_ptr` (or None) and `mirror_perm` (a
    host sequence of num_joints ints, or None) go together; `conf_ptr` (total_frames, num_joints) float32 over source frames or None;
    `state_ptr` (out_rows, num_joints) uint8 or None; `stats_ptr` (num_clips, num_joints, 4) int32 or None; `status_ptr` num_clips
    int32."""
    perm = _mirror_table("r3d_clips_repair", mirror_perm, num_joints)
    check(load().r3d_clips_repair(x_ptr, out_rows, num_joints, in_features, x_mirror_ptr or None, perm, table_ptr, num_clips, max_rows,
                                  conf_ptr or None, total_frames, min_conf, max_gap, state_ptr or None, stats_ptr or None, status_ptr, stream),
          "r3d_clips_repair")


def debug_clips_repair_host(x_ptr: int, out_rows: int, num_joints: int, in_features: int, x_mirror_ptr: Optional[int], mirror_perm,
                            table_ptr: int, num_clips: int, max_rows: int, conf_ptr: Optional[int], total_frames: int, min_conf: float,
                            max_gap: int, state_ptr: Optional[int], stats_ptr: Optional[int], status_ptr: int) -> int:
    """r3d_debug_clips_repair_host (hooks library only: use_hooks(True)): r3d_clips_repair on HOST pointers; `mirror_perm` a host
    sequence of ints of any length (the call judges it) or None; returns the status code instead of raising (R3D_ERR_ARG is what the
    tests ask for)."""
    perm = (C.c_int32 * max(len(mirror_perm), 1))(*[int(v) for v in mirror_perm]) if mirror_perm is not None else None
    return int(load().r3d_debug_clips_repair_host(x_ptr or None, out_rows, num_joints, in_features, x_mirror_ptr or None, perm,
                                                  table_ptr or None, num_clips, max_rows, conf_ptr or None, total_frames, min_conf, max_gap,
                                                  state_ptr or None, stats_ptr or None, status_ptr or None))


def clips_poses(raw_ptr: int, raw_mirror_ptr: Optional[int], raw_rows: int, num_joints: int, mirror_perm, table_ptr: int,
                raw_first_ptr: int, num_clips: int, max_frames: int, pred_ptr: Optional[int], world_ptr: Optional[int],
                total_frames: int, status_ptr: int, stream: int):
    """r3d_clips_poses: every pointer is device memory; `table_ptr` num_clips r3d_clip_desc (:func:`clip_desc_dtype`) back to
    back, `raw_first_ptr` num_clips int64; `raw_mirror_ptr` (or None) and `mirror_perm` (a host sequence of num_joints ints, or
    None) go together; `pred_ptr` / `world_ptr`: either may be None, not both; `status_ptr` num_clips int32."""
    perm = _mirror_table("r3d_clips_poses", mirror_perm, num_joints)
    check(load().r3d_clips_poses(raw_ptr, raw_mirror_ptr or None, raw_rows, num_joints, perm, table_ptr, raw_first_ptr, num_clips,
                                 max_frames, pred_ptr or None, world_ptr or None, total_frames, status_ptr, stream), "r3d_clips_poses")


def debug_clips_poses_host(raw_ptr: int, raw_mirror_ptr: Optional[int], raw_rows: int, num_joints: int, mirror_perm, table_ptr: int,
                           raw_first_ptr: int, num_clips: int, max_frames: int, pred_ptr: Optional[int], world_ptr: Optional[int],
                           total_frames: int, status_ptr: int) -> int:
    """r3d_debug_clips_poses_host (hooks library only: use_hooks(True)): r3d_clips_poses on HOST pointers; returns the status
    code instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    perm = _mirror_table("r3d_debug_clips_poses_host", mirror_perm, num_joints)
    return int(load().r3d_debug_clips_poses_host(raw_ptr, raw_mirror_ptr or None, raw_rows, num_joints, perm, table_ptr, raw_first_ptr,
                                                 num_clips, max_frames, pred_ptr or None, world_ptr or None, total_frames, status_ptr))


def clips_project(world_ptr: int, total_frames: int, num_joints: int, encoding: int, table_ptr: int, num_clips: int, max_rows: int,
                  x_ptr: int, out_rows: int, x_mirror_ptr: Optional[int], mirror_perm, gt_ptr: Optional[int], px_ptr: Optional[int],
                  gt_rows: int, outside_ptr: Optional[int], status_ptr: int, stream: int):
    """r3d_clips_project: every pointer is device memory; `table_ptr` num_clips r3d_clip_project_desc
    (:func:`clip_project_desc_dtype`) back to back; `x_mirror_ptr` (or None) and `mirror_perm` (a host sequence of num_joints
    ints, or None) go together; `gt_ptr` / `px_ptr` / `outside_ptr` may be None (`outside_ptr` is ADDED to: zero it first);
    `status_ptr` num_clips int32."""
    perm = _mirror_table("r3d_clips_project", mirror_perm, num_joints)
    check(load().r3d_clips_project(world_ptr, total_frames, num_joints, encoding, table_ptr, num_clips, max_rows, x_ptr, out_rows,
                                   x_mirror_ptr or None, perm, gt_ptr or None, px_ptr or None, gt_rows, outside_ptr or None,
                                   status_ptr, stream), "r3d_clips_project")


def debug_clips_project_host(world_ptr: int, total_frames: int, num_joints: int, encoding: int, table_ptr: int, num_clips: int,
                             max_rows: int, x_ptr: int, out_rows: int, x_mirror_ptr: Optional[int], mirror_perm,
                             gt_ptr: Optional[int], px_ptr: Optional[int], gt_rows: int, outside_ptr: Optional[int],
                             status_ptr: int) -> int:
    """r3d_debug_clips_project_host (hooks library only: use_hooks(True)): r3d_clips_project on HOST pointers; returns the
    status code instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    perm = _mirror_table("r3d_debug_clips_project_host", mirror_perm, num_joints)
    return int(load().r3d_debug_clips_project_host(world_ptr, total_frames, num_joints, encoding, table_ptr, num_clips, max_rows,
                                                   x_ptr, out_rows, x_mirror_ptr or None, perm, gt_ptr or None, px_ptr or None,
                                                   gt_rows, outside_ptr or None, status_ptr))


def clips_windows(src_ptr: int, total_frames: int, num_joints: int, in_features: int, receptive_field: int, runs_ptr: int,
                  num_runs: int, run_param_ptr: Optional[int], extrinsic_dim: int, window0: int, batch: int, x_ptr: int,
                  param_ptr: Optional[int], mirror_perm, status_ptr: int, stream: int):
    """r3d_clips_windows: every pointer is device memory; `runs_ptr` num_runs r3d_window_run_desc (:func:`window_run_dtype`) back
    to back; `run_param_ptr` (num_runs, extrinsic_dim) float32 and `param_ptr` (batch, extrinsic_dim) go together (both or None);
    `mirror_perm` a host sequence of num_joints ints, or None (then no run may flip); `status_ptr` num_runs int32."""
    perm = _mirror_table("r3d_clips_windows", mirror_perm, num_joints)
    check(load().r3d_clips_windows(src_ptr, total_frames, num_joints, in_features, receptive_field, runs_ptr, num_runs,
                                   run_param_ptr or None, extrinsic_dim, window0, batch, x_ptr, param_ptr or None, perm, status_ptr,
                                   stream), "r3d_clips_windows")


def debug_clips_windows_host(src_ptr: int, total_frames: int, num_joints: int, in_features: int, receptive_field: int, runs_ptr: int,
                             num_runs: int, run_param_ptr: Optional[int], extrinsic_dim: int, window0: int, batch: int, x_ptr: int,
                             param_ptr: Optional[int], mirror_perm, status_ptr: int) -> int:
    """r3d_debug_clips_windows_host (hooks library only: use_hooks(True)): r3d_clips_windows on HOST pointers; returns the status
    code instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    perm = _mirror_table("r3d_debug_clips_windows_host", mirror_perm, num_joints)
    return int(load().r3d_debug_clips_windows_host(src_ptr or None, total_frames, num_joints, in_features, receptive_field,
                                                   runs_ptr or None, num_runs, run_param_ptr or None, extrinsic_dim, window0, batch,
                                                   x_ptr or None, param_ptr or None, perm, status_ptr or None))


def streams_state_bytes(num_streams: int, receptive_field: int, num_joints: int, in_features: int) -> int:
    """r3d_streams_state_bytes: the bytes of the state r3d_streams_step keeps for `num_streams` streams - the heads, then the rings
    (0 for a shape the call refuses)."""
    return int(load().r3d_streams_state_bytes(num_streams, receptive_field, num_joints, in_features))


def streams_step(state_ptr: int, num_streams: int, receptive_field: int, lag: int, num_joints: int, in_features: int, encoding: int,
                 frame_ptr: int, cam_ptr: Optional[int], action_ptr: int, x_ptr: int, x_mirror_ptr: Optional[int], mirror_perm,
                 emit_ptr: int, status_ptr: int, stream: int):
    """r3d_streams_step: every pointer is device memory; `state_ptr` :func:`streams_state_bytes` bytes, 8-byte aligned; `cam_ptr`
    (num_streams, 16) float64 or None (R3D_ENCODE_NONE); `x_mirror_ptr` (or None) and `mirror_perm` (a host sequence of num_joints
    ints, or None) go together; `emit_ptr` num_streams int64, `status_ptr` num_streams int32."""
    perm = _mirror_table("r3d_streams_step", mirror_perm, num_joints)
    check(load().r3d_streams_step(state_ptr, num_streams, receptive_field, lag, num_joints, in_features, encoding, frame_ptr,
                                  cam_ptr or None, action_ptr, x_ptr, x_mirror_ptr or None, perm, emit_ptr, status_ptr, stream),
          "r3d_streams_step")


def debug_streams_step_host(state_ptr: int, num_streams: int, receptive_field: int, lag: int, num_joints: int, in_features: int,
                            encoding: int, frame_ptr: int, cam_ptr: Optional[int], action_ptr: int, x_ptr: int,
                            x_mirror_ptr: Optional[int], mirror_perm, emit_ptr: int, status_ptr: int) -> int:
    """r3d_debug_streams_step_host (hooks library only: use_hooks(True)): r3d_streams_step on HOST pointers; returns the status
    code instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    perm = _mirror_table("r3d_debug_streams_step_host", mirror_perm, num_joints)
    return int(load().r3d_debug_streams_step_host(state_ptr or None, num_streams, receptive_field, lag, num_joints, in_features, encoding,
                                                  frame_ptr or None, cam_ptr or None, action_ptr or None, x_ptr or None,
                                                  x_mirror_ptr or None, perm, emit_ptr or None, status_ptr or None))


def _streams_poses_features(what: str, in_features: int, reproj_ptr):
    """The residual is defined for ray inputs only; the C call has no in_features to check (x_dev is (S, RF, J, 3) by contract), so
    the binding refuses the other shape with the call's own code."""
    if reproj_ptr and in_features != 3:
        raise Ray3DHipError("%s failed (%d): reproj_dev is defined for 3-feature (ray) inputs only (in_features is %d)"
                            % (what, R3D_ERR_ARG, in_features))


def streams_poses(raw_ptr: int, raw_mirror_ptr: Optional[int], num_streams: int, num_joints: int, mirror_perm, emit_ptr: int,
                  status_ptr: int, desc_ptr: Optional[int], cam_ptr: Optional[int], x_ptr: Optional[int], receptive_field: int, lag: int,
                  pred_ptr: Optional[int], world_ptr: Optional[int], reproj_ptr: Optional[int], quality_ptr: Optional[int], stream: int,
                  in_features: int = 3):
    """r3d_streams_poses: every pointer is device memory; `raw_ptr` / `raw_mirror_ptr` (num_streams, num_joints, 3) float32;
    `raw_mirror_ptr` (or None) and `mirror_perm` (a host sequence of num_joints ints, or None) go together; `emit_ptr` /
    `status_ptr` the words r3d_streams_step wrote; `desc_ptr` num_streams r3d_stream_pose_desc (:func:`stream_pose_desc_dtype`);
    `cam_ptr` (num_streams, 16) float64 and `x_ptr` (num_streams, receptive_field, num_joints, 3) go with `reproj_ptr`; any of
    `pred_ptr`, `world_ptr`, `reproj_ptr` may be None, not all; `quality_ptr` only with `reproj_ptr`.  `in_features`: the width of
    the rows behind `x_ptr` - anything but 3 with `reproj_ptr` is refused here (R3D_ERR_ARG)."""
    _streams_poses_features("r3d_streams_poses", in_features, reproj_ptr)
    perm = _mirror_table("r3d_streams_poses", mirror_perm, num_joints)
    check(load().r3d_streams_poses(raw_ptr, raw_mirror_ptr or None, num_streams, num_joints, perm, emit_ptr, status_ptr, desc_ptr or None,
                                   cam_ptr or None, x_ptr or None, receptive_field, lag, pred_ptr or None, world_ptr or None,
                                   reproj_ptr or None, quality_ptr or None, stream), "r3d_streams_poses")


def debug_streams_poses_host(raw_ptr: int, raw_mirror_ptr: Optional[int], num_streams: int, num_joints: int, mirror_perm, emit_ptr: int,
                             status_ptr: int, desc_ptr: Optional[int], cam_ptr: Optional[int], x_ptr: Optional[int], receptive_field: int,
                             lag: int, pred_ptr: Optional[int], world_ptr: Optional[int], reproj_ptr: Optional[int],
                             quality_ptr: Optional[int]) -> int:
    """r3d_debug_streams_poses_host (hooks library only: use_hooks(True)): r3d_streams_poses on HOST pointers; returns the status
    code instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    perm = _mirror_table("r3d_debug_streams_poses_host", mirror_perm, num_joints)
    return int(load().r3d_debug_streams_poses_host(raw_ptr or None, raw_mirror_ptr or None, num_streams, num_joints, perm, emit_ptr or None,
                                                   status_ptr or None, desc_ptr or None, cam_ptr or None, x_ptr or None, receptive_field,
                                                   lag, pred_ptr or None, world_ptr or None, reproj_ptr or None, quality_ptr or None))


def streams_track_bytes(num_streams: int, receptive_field: int, num_joints: int, width: int) -> int:
    """r3d_streams_track_bytes: the bytes of the track r3d_streams_repair keeps for `num_streams` streams - (S, J) int32 ages,
    (S, J, width) float32 last inputs, (S, RF) uint32 masks, in that order (0 for a shape the call refuses).  `width`: 2 for the
    pixel encodings, in_features for R3D_ENCODE_NONE."""
    return int(load().r3d_streams_track_bytes(num_streams, receptive_field, num_joints, width))


def streams_repair(state_ptr: int, track_ptr: int, num_streams: int, receptive_field: int, lag: int, num_joints: int, in_features: int,
                   encoding: int, frame_ptr: int, conf_ptr: Optional[int], min_conf: float, cam_ptr: Optional[int], action_ptr: int,
                   max_gap: int, frame_out_ptr: int, synthetic_ptr: int, stream: int):
    """r3d_streams_repair (enqueued BEFORE :func:`streams_step` of the same tick, which is then given `frame_out_ptr` as its frame):
    every pointer is device memory; `state_ptr` the step's state; `track_ptr` :func:`streams_track_bytes` bytes, 8-byte aligned,
    all-zero = fresh; `conf_ptr` (num_streams, num_joints) float32 or None; `cam_ptr` (num_streams, 16) float64 or None
    (R3D_ENCODE_NONE); `synthetic_ptr` num_streams uint32."""
    check(load().r3d_streams_repair(state_ptr, track_ptr, num_streams, receptive_field, lag, num_joints, in_features, encoding, frame_ptr,
                                    conf_ptr or None, min_conf, cam_ptr or None, action_ptr, max_gap, frame_out_ptr, synthetic_ptr, stream),
          "r3d_streams_repair")


def debug_streams_repair_host(state_ptr: int, track_ptr: int, num_streams: int, receptive_field: int, lag: int, num_joints: int,
                              in_features: int, encoding: int, frame_ptr: int, conf_ptr: Optional[int], min_conf: float,
                              cam_ptr: Optional[int], action_ptr: int, max_gap: int, frame_out_ptr: int, synthetic_ptr: int) -> int:
    """r3d_debug_streams_repair_host (hooks library only: use_hooks(True)): r3d_streams_repair on HOST pointers; returns the status
    code instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    return int(load().r3d_debug_streams_repair_host(state_ptr or None, track_ptr or None, num_streams, receptive_field, lag, num_joints,
                                                    in_features, encoding, frame_ptr or None, conf_ptr or None, min_conf, cam_ptr or None,
                                                    action_ptr or None, max_gap, frame_out_ptr or None, synthetic_ptr or None))


def _looks_table(looks):
    """The host array of looks r3d_streams_peek takes (any length: the call judges it)."""
    looks = [int(v) for v in looks]
    return (C.c_int32 * max(len(looks), 1))(*looks), len(looks)


def streams_peek(state_ptr: int, num_streams: int, receptive_field: int, lag: int, num_joints: int, in_features: int, looks,
                 action_ptr: Optional[int], status_ptr: int, x_ptr: int, x_mirror_ptr: Optional[int], mirror_perm, emit_ptr: int,
                 peek_status_ptr: int, stream: int):
    """r3d_streams_peek (enqueued AFTER :func:`streams_step` of the same tick): every pointer is device memory; `state_ptr` the
    step's state, read only; `looks` a host sequence of 1..STREAMS_PEEK_MAX strictly increasing ints in [0, lag); `action_ptr`
    (or None: every stream counts as pushed) and `status_ptr` the step's words; `x_ptr` / `x_mirror_ptr` (len(looks), num_streams,
    receptive_field, num_joints, in_features) float32, `x_mirror_ptr` (or None) and `mirror_perm` go together; `emit_ptr`
    (len(looks), num_streams) int64, `peek_status_ptr` the same shape int32."""
    perm = _mirror_table("r3d_streams_peek", mirror_perm, num_joints)
    table, n = _looks_table(looks)
    check(load().r3d_streams_peek(state_ptr, num_streams, receptive_field, lag, num_joints, in_features, table, n, action_ptr or None,
                                  status_ptr, x_ptr, x_mirror_ptr or None, perm, emit_ptr, peek_status_ptr, stream), "r3d_streams_peek")


def debug_streams_peek_host(state_ptr: int, num_streams: int, receptive_field: int, lag: int, num_joints: int, in_features: int, looks,
                            action_ptr: Optional[int], status_ptr: int, x_ptr: int, x_mirror_ptr: Optional[int], mirror_perm,
                            emit_ptr: int, peek_status_ptr: int, num_looks: Optional[int] = None) -> int:
    """r3d_debug_streams_peek_host (hooks library only: use_hooks(True)): r3d_streams_peek on HOST pointers; returns the status
    code instead of raising (R3D_ERR_ARG is what the tests ask for).  `looks` None: a null pointer; `num_looks` overrides the
    sequence's length."""
    perm = _mirror_table("r3d_debug_streams_peek_host", mirror_perm, num_joints)
    table, n = _looks_table(looks) if looks is not None else (None, 0)
    return int(load().r3d_debug_streams_peek_host(state_ptr or None, num_streams, receptive_field, lag, num_joints, in_features, table,
                                                  n if num_looks is None else num_looks, action_ptr or None, status_ptr or None,
                                                  x_ptr or None, x_mirror_ptr or None, perm, emit_ptr or None, peek_status_ptr or None))


def streams_fuse(world_ptr: int, reproj_ptr: Optional[int], emit_ptr: int, status_ptr: int, synthetic_ptr: Optional[int], num_streams: int,
                 num_joints: int, member_ptr: int, num_groups: int, max_members: int, soft_px: float, max_px: float, max_dist: float,
                 fused_ptr: int, spread_ptr: Optional[int], count_ptr: Optional[int], used_ptr: Optional[int], stream: int):
    """r3d_streams_fuse (enqueued AFTER :func:`streams_poses` of the same tick): every pointer is device memory; `world_ptr`
    (num_streams, num_joints, 3) float64 and `reproj_ptr` (num_streams, num_joints) float64 or None what r3d_streams_poses wrote;
    `emit_ptr` / `status_ptr` the step's words; `synthetic_ptr` r3d_streams_repair's mask words or None; `member_ptr` (num_groups,
    max_members) int32 stream indices, negative: an empty slot, max_members <= FUSE_MAX_MEMBERS; `fused_ptr` (num_groups,
    num_joints, 3) float64; `spread_ptr` (num_groups, num_joints) float64, `count_ptr` the same shape int32 and `used_ptr`
    (num_groups, max_members) uint32, each or None."""
    check(load().r3d_streams_fuse(world_ptr, reproj_ptr or None, emit_ptr, status_ptr, synthetic_ptr or None, num_streams, num_joints,
                                  member_ptr, num_groups, max_members, soft_px, max_px, max_dist, fused_ptr, spread_ptr or None,
                                  count_ptr or None, used_ptr or None, stream), "r3d_streams_fuse")


def debug_streams_fuse_host(world_ptr: int, reproj_ptr: Optional[int], emit_ptr: int, status_ptr: int, synthetic_ptr: Optional[int],
                            num_streams: int, num_joints: int, member_ptr: int, num_groups: int, max_members: int, soft_px: float,
                            max_px: float, max_dist: float, fused_ptr: int, spread_ptr: Optional[int], count_ptr: Optional[int],
                            used_ptr: Optional[int]) -> int:
    """r3d_debug_streams_fuse_host (hooks library only: use_hooks(True)): r3d_streams_fuse on HOST pointers; returns the status
    code instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    return int(load().r3d_debug_streams_fuse_host(world_ptr or None, reproj_ptr or None, emit_ptr or None, status_ptr or None,
                                                  synthetic_ptr or None, num_streams, num_joints, member_ptr or None, num_groups,
                                                  max_members, soft_px, max_px, max_dist, fused_ptr or None, spread_ptr or None,
                                                  count_ptr or None, used_ptr or None))


class AssignParams(C.Structure):
    """r3d_assign_params (include/ray3d_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("num_cameras", C.c_int32), ("slots", C.c_int32), ("max_detections", C.c_int32),
                ("num_joints", C.c_int32), ("width", C.c_int32), ("lag", C.c_int32), ("min_joints", C.c_int32), ("min_common", C.c_int32),
                ("max_missed", C.c_int32), ("fill", C.c_int32), ("min_conf", C.c_float), ("max_cost", C.c_double)]


def assign_params(num_cameras: int, slots: int, max_detections: int, num_joints: int, width: int, lag: int, min_joints: int,
                  min_common: int, max_missed: int, fill: int, min_conf: float, max_cost: float) -> AssignParams:
    """An r3d_assign_params with its struct_size set."""
    return AssignParams(C.sizeof(AssignParams), num_cameras, slots, max_detections, num_joints, width, lag, min_joints, min_common,
                        max_missed, fill, min_conf, max_cost)


def streams_assign_bytes(num_cameras: int, slots: int, num_joints: int, width: int) -> int:
    """r3d_streams_assign_bytes: bytes of the state of r3d_streams_assign (all zero = no tracks); 0 for shapes the call refuses."""
    return int(load().r3d_streams_assign_bytes(num_cameras, slots, num_joints, width))


def streams_assign(state_ptr: int, prm: AssignParams, det_ptr: int, det_conf_ptr: Optional[int], det_count_ptr: int, action_ptr: int,
                   frame_out_ptr: int, conf_out_ptr: Optional[int], match_ptr: int, id_ptr: int, stats_ptr: Optional[int], stream: int):
    """r3d_streams_assign (enqueued BEFORE :func:`streams_repair` / :func:`streams_step` of the same tick): every pointer is device
    memory but `prm` (:func:`assign_params`); `det_ptr` (C, D, J, width) float32, `det_conf_ptr` (C, D, J) float32 or None,
    `det_count_ptr` (C,) int32; written: `action_ptr` (S,) int32, `frame_out_ptr` (S, J, width) float32, `conf_out_ptr` (S, J) float32
    or None, `match_ptr` (S,) int32, `id_ptr` (S,) int64, `stats_ptr` (C, 4) int32 or None, S = C * P."""
    check(load().r3d_streams_assign(state_ptr, C.byref(prm), det_ptr, det_conf_ptr or None, det_count_ptr, action_ptr, frame_out_ptr,
                                    conf_out_ptr or None, match_ptr, id_ptr, stats_ptr or None, stream), "r3d_streams_assign")


def debug_streams_assign_host(state_ptr: Optional[int], prm: Optional[AssignParams], det_ptr: Optional[int], det_conf_ptr: Optional[int],
                              det_count_ptr: Optional[int], action_ptr: Optional[int], frame_out_ptr: Optional[int],
                              conf_out_ptr: Optional[int], match_ptr: Optional[int], id_ptr: Optional[int], stats_ptr: Optional[int]) -> int:
    """r3d_debug_streams_assign_host (hooks library only: use_hooks(True)): r3d_streams_assign on HOST pointers; returns the status
    code instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    return int(load().r3d_debug_streams_assign_host(state_ptr or None, C.byref(prm) if prm is not None else None, det_ptr or None,
                                                    det_conf_ptr or None, det_count_ptr or None, action_ptr or None, frame_out_ptr or None,
                                                    conf_out_ptr or None, match_ptr or None, id_ptr or None, stats_ptr or None))


class LinkParams(C.Structure):
    """r3d_link_params (include/ray3d_hip.h)."""
    _fields_ = [("struct_size", C.c_int32), ("num_scenes", C.c_int32), ("num_cameras", C.c_int32), ("slots", C.c_int32),
                ("people", C.c_int32), ("max_members", C.c_int32), ("num_joints", C.c_int32), ("min_joints", C.c_int32),
                ("min_common", C.c_int32), ("max_missed", C.c_int32), ("max_dist", C.c_double), ("break_dist", C.c_double)]


def link_params(num_scenes: int, num_cameras: int, slots: int, people: int, max_members: int, num_joints: int, min_joints: int,
                min_common: int, max_missed: int, max_dist: float, break_dist: float = 0.0) -> LinkParams:
    """An r3d_link_params with its struct_size set."""
    return LinkParams(C.sizeof(LinkParams), num_scenes, num_cameras, slots, people, max_members, num_joints, min_joints, min_common,
                      max_missed, max_dist, break_dist)


def streams_link_bytes(num_scenes: int, num_cameras: int, people: int, num_joints: int) -> int:
    """r3d_streams_link_bytes: bytes of the state of r3d_streams_link (all zero = no people); 0 for shapes the call refuses."""
    return int(load().r3d_streams_link_bytes(num_scenes, num_cameras, people, num_joints))


def streams_link(state_ptr: int, prm: LinkParams, world_ptr: int, emit_ptr: int, status_ptr: int, id_ptr: int, member_ptr: int,
                 person_ptr: int, group_ptr: Optional[int], stats_ptr: Optional[int], stream: int):
    """r3d_streams_link (enqueued BEHIND :func:`streams_poses` and BEFORE :func:`streams_fuse` of the same tick): every pointer is
    device memory but `prm` (:func:`link_params`); `world_ptr` (S, J, 3) float64, `emit_ptr` (S,) int64, `status_ptr` (S,) int32,
    `id_ptr` (S,) int64 track identities; written: `member_ptr` (N * G, M) int32 - the member table of :func:`streams_fuse` -,
    `person_ptr` (N * G,) int64, `group_ptr` (S,) int32 or None, `stats_ptr` (N, 4) int32 or None, S = N * C * P."""
    check(load().r3d_streams_link(state_ptr, C.byref(prm), world_ptr, emit_ptr, status_ptr, id_ptr, member_ptr, person_ptr,
                                  group_ptr or None, stats_ptr or None, stream), "r3d_streams_link")


def debug_streams_link_host(state_ptr: Optional[int], prm: Optional[LinkParams], world_ptr: Optional[int], emit_ptr: Optional[int],
                            status_ptr: Optional[int], id_ptr: Optional[int], member_ptr: Optional[int], person_ptr: Optional[int],
                            group_ptr: Optional[int], stats_ptr: Optional[int]) -> int:
    """r3d_debug_streams_link_host (hooks library only: use_hooks(True)): r3d_streams_link on HOST pointers; returns the status code
    instead of raising (R3D_ERR_ARG is what the tests ask for)."""
    return int(load().r3d_debug_streams_link_host(state_ptr or None, C.byref(prm) if prm is not None else None, world_ptr or None,
                                                  emit_ptr or None, status_ptr or None, id_ptr or None, member_ptr or None,
                                                  person_ptr or None, group_ptr or None, stats_ptr or None))


def _census_rows(call):
    cap = 256
    while True:
        rows = (CensusRow * cap)()
        n = call(rows, cap)
        if n < 0:
            raise Ray3DHipError("census failed (%d): %s" % (n, load().r3d_last_error().decode()))
        if n <= cap:
            return [(r.launch, r.kernel.decode(), r.blocks, r.tile_kind.decode(), r.tiles) for r in rows[:n]]
        cap = n


def debug_forward_census(pos: Optional[Handle], trj: Optional[Handle], batch: int, window_stride: int, nwg: int = 256, uv: bool = False,
                         cam_stride: int = 0, staged: bool = False, captured: bool = False):
    """r3d_debug_forward_census (hooks library only: use_hooks(True)): the launches one forward of `batch` windows would make, as a
    list of ``(kernel, blocks, {tile kind: tiles})`` in launch order - host only.  `window_stride` in frames (RF: independent
    windows; 1: a clip call), `cam_stride` as r3d_input's (0: one camera row)."""
    lib = _lib_of(pos, trj)
    ws = int(window_stride)
    rows = _census_rows(lambda r, cap: lib.r3d_debug_forward_census(pos.ptr if pos else None, trj.ptr if trj else None, batch, nwg,
                                                                   1 if uv else 0, cam_stride, ws, 1 if staged else 0,
                                                                   1 if captured else 0, r, cap))
    launches = []
    for launch, kernel, blocks, kind, tiles in rows:
        if launch == len(launches):
            launches.append((kernel, blocks, {}))
        if kind:
            launches[launch][2][kind] = tiles
    return launches


def debug_census_domain():
    """r3d_debug_census_domain (hooks library only): ``(kernel names a launch record can carry, {(kernel, tile kind)} the persistent
    loop's dispatch instantiates)``."""
    lib = load()
    rows = _census_rows(lambda r, cap: lib.r3d_debug_census_domain(r, cap))
    return [k for _, k, _, kind, _ in rows if not kind], {(k, kind) for _, k, _, kind, _ in rows if kind}


def debug_plan_kind_edges():
    """r3d_debug_plan_kind_edges (hooks library only): the largest window count of every plan kind that has one, ascending."""
    lib = load()
    buf = (C.c_int64 * 8)()
    n = lib.r3d_debug_plan_kind_edges(buf, 8)
    if n < 0 or n > 8:
        raise Ray3DHipError("r3d_debug_plan_kind_edges returned %d" % n)
    return [int(v) for v in buf[:n]]


def debug_plan_buffers(pos: Optional[Handle], trj: Optional[Handle], batch: int):
    """r3d_debug_plan_buffers (hooks library only: use_hooks(True)): ``(rows, workspace_bytes)`` of a call of `batch` windows - rows
    ``(name, floats_per_window, offset_bytes, bytes, per_frame)`` in workspace order, the plan's buffers then "(tail)" and
    "(control)"; `workspace_bytes` their sum.  Host only."""
    lib = _lib_of(pos, trj)
    cap = 128
    while True:
        rows = (PlanBufferRow * cap)()
        total = C.c_uint64()
        n = lib.r3d_debug_plan_buffers(pos.ptr if pos else None, trj.ptr if trj else None, int(batch), rows, cap, C.byref(total))
        if n < 0:
            raise Ray3DHipError("r3d_debug_plan_buffers returned %d" % n)
        if n <= cap:
            return [(r.name.decode(), int(r.floats_per_window), int(r.offset_bytes), int(r.bytes), bool(r.per_frame)) for r in rows[:n]], int(total.value)
        cap = n


def debug_call_check(pos: Optional[Handle], trj: Optional[Handle], batch: int, window_stride: int, mode: int = R3D_INPUT_RAYS,
                     cam_stride: int = 0):
    """r3d_debug_call_check (hooks library only: use_hooks(True)): ``(code, message, per_frame)`` - what a forward of this shape
    answers to its size limits (0 and "" when it is accepted) and whether it would run the per-frame first layers.  Host only."""
    lib = _lib_of(pos, trj)
    pf = C.c_int32()
    rc = int(lib.r3d_debug_call_check(pos.ptr if pos else None, trj.ptr if trj else None, int(mode), int(window_stride), int(cam_stride),
                                      int(batch), C.byref(pf)))
    return rc, (lib.r3d_last_error().decode() if rc != 0 else ""), bool(pf.value)


def _parent_table(parents):
    return (C.c_int32 * len(parents))(*[int(v) for v in parents]) if parents is not None else None


def clip_valid_losses(pos_ptr: int, trj_ptr: Optional[int], gt_ptr: int, n_frames: int, num_joints: int, parents,
                      flags: int, out_ptr: int, frame_ptr: Optional[int], stream: int):
    """r3d_clip_valid_losses: `parents` a host sequence of at least num_joints ints (or None: no bone terms), `out_ptr`
    VALID_OUT_DOUBLES float64 of device memory (the first VALID_DOUBLES are the results), `frame_ptr` (n_frames, VALID_COUNT)
    float64 or None; the rest device pointers."""
    check(load().r3d_clip_valid_losses(pos_ptr, trj_ptr or None, gt_ptr, n_frames, num_joints, _parent_table(parents), flags,
                                       out_ptr, frame_ptr or None, stream), "r3d_clip_valid_losses")


def clips_valid_scratch_bytes(num_clips: int, max_frames: int) -> int:
    """r3d_clips_valid_scratch_bytes: the scratch one r3d_clips_valid_losses call over `num_clips` clips of at most `max_frames`
    frames needs (0 for num_clips < 1 or max_frames < 1)."""
    return int(load().r3d_clips_valid_scratch_bytes(num_clips, max_frames))


def clips_valid_losses(pos_ptr: int, trj_ptr: Optional[int], gt_ptr: int, total_frames: int, num_joints: int, parents, flags: int,
                       table_ptr: int, num_clips: int, max_frames: int, rows_ptr: int, row_stride: int, frame_ptr: Optional[int],
                       scratch_ptr: int, scratch_bytes: int, stream: int):
    """r3d_clips_valid_losses: every pointer but `parents` (a host sequence of at least num_joints ints, or None: no bone terms) is
    device memory; `table_ptr` num_clips r3d_clip_desc (:func:`clip_desc_dtype`) back to back, their rn2w / tn2w unread;
    `trj_ptr` / `frame_ptr` may be None."""
    check(load().r3d_clips_valid_losses(pos_ptr, trj_ptr or None, gt_ptr, total_frames, num_joints, _parent_table(parents), flags,
                                        table_ptr, num_clips, max_frames, rows_ptr, row_stride, frame_ptr or None, scratch_ptr,
                                        scratch_bytes, stream), "r3d_clips_valid_losses")


def forward_pair(pos: Handle, trj: Handle, inp: Input, batch: int, out_ptr: int,
                 out_trj_ptr: Optional[int], ws_ptr: int, ws_bytes: int, stream: int):
    check(pos._lib.r3d_forward_pair(pos.ptr, trj.ptr, C.byref(inp), batch, out_ptr, out_trj_ptr,
                                  ws_ptr, ws_bytes, stream), "r3d_forward_pair")


def forward_pair_split(pos: Handle, trj: Handle, inp: Input, batch: int, out_pos_ptr: int,
                       out_trj_ptr: int, ws_ptr: int, ws_bytes: int, stream: int):
    """r3d_forward_pair_split: r3d_forward_pair with the pos network's output and the trajectory kept apart (both required)."""
    check(pos._lib.r3d_forward_pair_split(pos.ptr, trj.ptr, C.byref(inp), batch, out_pos_ptr, out_trj_ptr,
                                        ws_ptr, ws_bytes, stream), "r3d_forward_pair_split")
