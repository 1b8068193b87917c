"""ctypes binding of libsrlhip.so (include/srlhip.h).

The HIP library is the product: there is NO CPU fallback.  If the shared
object is missing or no MI355X is visible, the errors raised here say so.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SRLHIP_LIB") or os.path.join(HERE, "libsrlhip.so")      # SRLHIP_LIB: experiment builds (profiles/probes)

# ---- constants mirrored from include/srlhip.h --------------------------------
ENV_MOBILE, ENV_MOBILE_1D, ENV_MOBILE_2TARGET, ENV_MOBILE_LINE, ENV_KUKA_BUTTON, ENV_KUKA_MOVING, ENV_KUKA_2BUTTON, ENV_KUKA_RAND = range(8)
OBS_GROUND_TRUTH, OBS_JOINTS, OBS_JOINTS_POSITION, OBS_RAW_PIXELS = range(4)
RNG_HOST, RNG_PHILOX, RNG_MT19937 = range(3)
F_POS_X, F_POS_Y, F_TARGET_X, F_TARGET_Y, F_STEP_COUNT, F_CUR_TARGET, F_LAST_REWARD, F_EP_RETURN, F_EP_LENGTH = range(9)
F_TARGET2_X, F_TARGET2_Y = 9, 10
F_LAST_RETURN, F_LAST_LENGTH, F_N_FINISHED = 11, 12, 13
F_KUKA_Q, F_KUKA_QD, F_KUKA_EE_TARGET, F_KUKA_BUTTON_Q, F_KUKA_BUTTON_POS, F_KUKA_GRIPPER, F_KUKA_COUNTERS = range(16, 23)
F_KUKA_BUTTON_XY, F_KUKA_BUTTON2_Q, F_KUKA_BUTTON2_XY, F_KUKA_GOAL, F_KUKA_OBJECTS, F_KUKA_GRIPPER_Q, F_KUKA_GRIPPER_QD, F_KUKA_BODIES, F_KUKA_IK_CROSSED = range(23, 32)
KUKA_MODEL_LUMPED, KUKA_MODEL_FULL = 0, 1          # srlhip_config.kuka_model

_FIELD_SHAPES = {
    F_POS_X: (np.float64, 1), F_POS_Y: (np.float64, 1), F_TARGET_X: (np.float64, 1), F_TARGET_Y: (np.float64, 1),
    F_STEP_COUNT: (np.int32, 1), F_CUR_TARGET: (np.int32, 1), F_LAST_REWARD: (np.float64, 1),
    F_EP_RETURN: (np.float64, 1), F_EP_LENGTH: (np.int32, 1), F_TARGET2_X: (np.float64, 1), F_TARGET2_Y: (np.float64, 1),
    F_LAST_RETURN: (np.float64, 1), F_LAST_LENGTH: (np.int32, 1), F_N_FINISHED: (np.int32, 1),
    F_KUKA_Q: (np.float64, 7), F_KUKA_QD: (np.float64, 7), F_KUKA_EE_TARGET: (np.float64, 3),
    F_KUKA_BUTTON_Q: (np.float64, 2), F_KUKA_BUTTON_POS: (np.float64, 3), F_KUKA_GRIPPER: (np.float64, 3),
    F_KUKA_COUNTERS: (np.int32, 3), F_KUKA_BUTTON_XY: (np.float64, 2), F_KUKA_BUTTON2_Q: (np.float64, 2),
    F_KUKA_BUTTON2_XY: (np.float64, 2), F_KUKA_GOAL: (np.int32, 2), F_KUKA_OBJECTS: (np.float64, 30),
    F_KUKA_GRIPPER_Q: (np.float64, 5), F_KUKA_GRIPPER_QD: (np.float64, 5), F_KUKA_BODIES: (np.float64, 66), F_KUKA_IK_CROSSED: (np.int32, 1),
}

EXPORTS = [
    "srlhip_abi_version", "srlhip_default_config", "srlhip_create", "srlhip_destroy", "srlhip_obs_dim",
    "srlhip_obs_bytes", "srlhip_action_dim", "srlhip_num_actions", "srlhip_seed", "srlhip_reset",
    "srlhip_reset_rand_count", "srlhip_step", "srlhip_step_async", "srlhip_step_wait", "srlhip_step_pending", "srlhip_set_persistent", "srlhip_rollout", "srlhip_rollout_policy", "srlhip_rollout_policy_sampled", "srlhip_sample_actions", "srlhip_rollout_mlp_policy", "srlhip_rollout_mlp_policy_sampled", "srlhip_rollout_policy_summary", "srlhip_policy_act", "srlhip_cnn_policy_act", "srlhip_cnn_param_count", "srlhip_pixel_policy_act", "srlhip_get_state", "srlhip_set_state",
    "srlhip_device_ptr", "srlhip_render", "srlhip_episode_stats", "srlhip_episode_records", "srlhip_episode_stats_device", "srlhip_sync", "srlhip_copy_async", "srlhip_stream", "srlhip_timing_begin",
    "srlhip_timing_end", "srlhip_last_error", "srlhip_selftest_group_primitives", "srlhip_selftest_rng", "srlhip_kuka_kernel", "srlhip_kuka_default_model", "srlhip_set_kuka_model", "srlhip_kuka_tree_default_model", "srlhip_set_kuka_tree_model",
    "srlhip_graph_begin", "srlhip_graph_end", "srlhip_graph_launch", "srlhip_graph_destroy",
    "srlhip_encoder_supported", "srlhip_encoder_feature_count", "srlhip_encoder_create", "srlhip_encoder_forward", "srlhip_encoder_overflow",
    "srlhip_encoder_phase_cycles",
    "srlhip_encoder_destroy", "srlhip_encoder_last_error", "srlhip_encoder_pack_bytes", "srlhip_encoder_pack", "srlhip_encoder_pack_i8_bytes", "srlhip_encoder_pack_i8", "srlhip_encoder_pack_first_layer",
    "srlhip_jpeg_encode", "srlhip_render_jpeg", "srlhip_jpeg_header_bytes", "srlhip_jpeg_encode_host",
    "srlhip_jpeg_probe", "srlhip_jpeg_decode_host", "srlhip_jpeg_decode_workspace_bytes", "srlhip_jpeg_decode",
    "srlhip_jpeg_probe_baseline", "srlhip_jpeg_decode_baseline_host", "srlhip_jpeg_decode_baseline_workspace_bytes", "srlhip_jpeg_decode_baseline",
    "srlhip_pca_supported", "srlhip_pca_create", "srlhip_pca_forward", "srlhip_pca_project_host", "srlhip_pca_destroy", "srlhip_pca_last_error",
    "srlhip_pca_gram_supported", "srlhip_pca_gram", "srlhip_pca_gram_host", "srlhip_pca_gram_last_error",
    "srlhip_knn_supported", "srlhip_knn_workspace_bytes", "srlhip_knn", "srlhip_knn_host", "srlhip_knn_last_error",
    "srlhip_linear_srl_supported", "srlhip_linear_srl_workspace_bytes", "srlhip_linear_srl_forward", "srlhip_linear_srl_step",
    "srlhip_linear_srl_forward_host", "srlhip_linear_srl_step_host", "srlhip_linear_srl_last_error",
]


ABI_VERSION = 5
KUKA_MODEL_DOUBLES = 138
KUKA_TREE_MODEL_DOUBLES = 510
KUKA_DETAIL_ALT_SWEEP, KUKA_DETAIL_BODY_ORDER, KUKA_DETAIL_FRICTION2 = 1, 2, 4


def kuka_tree_default_model():
    """The baked srlhip_kuka_tree_model (full 12-DoF gripper tree) as a flat float64[510] (no GPU needed)."""
    t = np.zeros(KUKA_TREE_MODEL_DOUBLES)
    rc = load().srlhip_kuka_tree_default_model(t.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return t


def kuka_default_model():
    """The baked srlhip_kuka_model as a flat float64[138] (no GPU needed)."""
    t = np.zeros(KUKA_MODEL_DOUBLES)
    rc = load().srlhip_kuka_default_model(t.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return t


class Config(ctypes.Structure):
    """struct srlhip_config"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("env_kind", ctypes.c_int32), ("num_envs", ctypes.c_int32),
        ("device_id", ctypes.c_int32), ("first_env_id", ctypes.c_int32), ("is_discrete", ctypes.c_int32),
        ("random_target", ctypes.c_int32), ("force_down", ctypes.c_int32), ("shape_reward", ctypes.c_int32),
        ("action_repeat", ctypes.c_int32), ("action_joints", ctypes.c_int32), ("obs_mode", ctypes.c_int32),
        ("img_h", ctypes.c_int32), ("img_w", ctypes.c_int32), ("multi_view", ctypes.c_int32),
        ("rng_mode", ctypes.c_int32), ("auto_reset", ctypes.c_int32), ("io_device", ctypes.c_int32),
        ("kuka_model", ctypes.c_int32), ("info_bits", ctypes.c_int32),
        ("seed0", ctypes.c_int64), ("max_distance", ctypes.c_double),
    ]


class LinearPolicy(ctypes.Structure):
    """struct srlhip_linear_policy"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("per_env", ctypes.c_int32), ("freeze_after_done", ctypes.c_int32),
        ("normalize", ctypes.c_int32), ("weights", ctypes.c_void_p), ("obs_mean", ctypes.c_void_p),
        ("obs_std", ctypes.c_void_p), ("clip_obs", ctypes.c_double),
    ]


class MlpPolicy(ctypes.Structure):
    """struct srlhip_mlp_policy"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("per_env", ctypes.c_int32), ("freeze_after_done", ctypes.c_int32),
        ("normalize", ctypes.c_int32), ("hidden", ctypes.c_int32), ("reserved", ctypes.c_int32), ("params", ctypes.c_void_p),
        ("obs_mean", ctypes.c_void_p), ("obs_std", ctypes.c_void_p), ("clip_obs", ctypes.c_double),
    ]


class RolloutSummary(ctypes.Structure):
    """struct srlhip_rollout_summary"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("ret", ctypes.c_void_p), ("length", ctypes.c_void_p),
        ("obs_sum", ctypes.c_void_p), ("obs_sqsum", ctypes.c_void_p),
    ]


class CnnPolicy(ctypes.Structure):
    """struct srlhip_cnn_policy"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("per_env", ctypes.c_int32), ("freeze_after_done", ctypes.c_int32),
        ("reserved", ctypes.c_int32), ("params", ctypes.c_void_p),
    ]


class PixelPolicy(ctypes.Structure):
    """struct srlhip_pixel_policy"""
    _fields_ = [
        ("struct_size", ctypes.c_int32), ("paired", ctypes.c_int32), ("freeze_after_done", ctypes.c_int32),
        ("reserved", ctypes.c_int32), ("weights", ctypes.c_void_p), ("delta", ctypes.c_void_p), ("noise", ctypes.c_double),
    ]


class SrlHipError(RuntimeError):
    pass


_lib = None


def load():
    """dlopen libsrlhip.so; raises (never falls back) when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SrlHipError(
            "libsrlhip.so is not built ({}). Run `python -c 'import __graft_entry__ as g; g.build()'` or "
            "`make -C robotics-rl-srl_amd/csrc`. There is no CPU fallback for the env stepper.".format(LIB_PATH))
    # PyTorch ships its own libamdhip64.so; the first HIP runtime loaded serves the whole process and torch cannot see
    # the GPU through /opt/rocm's copy.  When torch is installed, let it load its runtime first (libsrlhip.so works with either).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    if lib.srlhip_abi_version() != ABI_VERSION:       # a stale build next to a newer host package (table sizes, field ids) must not be driven
        raise SrlHipError("libsrlhip.so reports ABI version {}, this host package needs {}: rebuild it "
                          "(make -C robotics-rl-srl_amd/csrc)".format(lib.srlhip_abi_version(), ABI_VERSION))
    lib.srlhip_last_error.restype = ctypes.c_char_p
    lib.srlhip_last_error.argtypes = [vp]
    lib.srlhip_default_config.argtypes = [i32, ctypes.POINTER(Config)]
    lib.srlhip_create.argtypes = [ctypes.POINTER(Config), ctypes.POINTER(vp)]
    for name in ("srlhip_destroy", "srlhip_obs_dim", "srlhip_obs_bytes", "srlhip_action_dim", "srlhip_num_actions",
                 "srlhip_reset_rand_count", "srlhip_sync", "srlhip_timing_begin", "srlhip_step_pending"):
        getattr(lib, name).argtypes = [vp]
    lib.srlhip_seed.argtypes = [vp, vp, vp]
    lib.srlhip_reset.argtypes = [vp, vp, vp, vp]
    lib.srlhip_step.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.srlhip_step_async.argtypes = [vp, vp, vp]
    lib.srlhip_step_wait.argtypes = [vp, vp, vp, vp]
    lib.srlhip_set_persistent.argtypes = [vp, i32, i32]
    lib.srlhip_rollout.argtypes = [vp, i32, vp, vp, vp, vp, vp]
    lib.srlhip_rollout_policy.argtypes = [vp, i32, ctypes.POINTER(LinearPolicy), vp, vp, vp, vp]
    lib.srlhip_rollout_policy_sampled.argtypes = [vp, i32, ctypes.POINTER(LinearPolicy), vp, vp, vp, vp]
    lib.srlhip_sample_actions.argtypes = [vp, vp, vp, vp]
    lib.srlhip_rollout_mlp_policy.argtypes = [vp, i32, ctypes.POINTER(MlpPolicy), vp, vp, vp, vp]
    lib.srlhip_rollout_mlp_policy_sampled.argtypes = [vp, i32, ctypes.POINTER(MlpPolicy), vp, vp, vp, vp]
    lib.srlhip_rollout_policy_summary.argtypes = [vp, i32, ctypes.POINTER(LinearPolicy), ctypes.POINTER(MlpPolicy), i32, ctypes.POINTER(RolloutSummary)]
    lib.srlhip_policy_act.argtypes = [vp, ctypes.POINTER(LinearPolicy), ctypes.POINTER(MlpPolicy), i32, vp, i32, vp, vp, vp, vp]
    lib.srlhip_cnn_policy_act.argtypes = [vp, ctypes.POINTER(CnnPolicy), i32, vp, vp, vp, vp, vp]
    lib.srlhip_pixel_policy_act.argtypes = [vp, ctypes.POINTER(PixelPolicy), vp, vp, vp, vp, vp]
    lib.srlhip_cnn_param_count.argtypes = [i32, i32, i32, i32]
    lib.srlhip_cnn_param_count.restype = ctypes.c_int64
    lib.srlhip_get_state.argtypes = [vp, i32, vp]
    lib.srlhip_set_state.argtypes = [vp, i32, vp]
    lib.srlhip_device_ptr.argtypes = [vp, i32, ctypes.POINTER(vp)]
    lib.srlhip_episode_stats.argtypes = [vp, vp, vp, vp]
    lib.srlhip_episode_stats_device.argtypes = [vp, vp, vp, vp]
    lib.srlhip_episode_records.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    lib.srlhip_selftest_group_primitives.argtypes = [i32, vp, vp, i32]
    lib.srlhip_selftest_rng.argtypes = [i32] * 5 + [vp] * 5 + [i32, vp, i32, vp, vp, ctypes.c_int64, vp, ctypes.c_int64]
    lib.srlhip_kuka_kernel.argtypes = [vp]
    lib.srlhip_kuka_default_model.argtypes = [vp]
    lib.srlhip_set_kuka_model.argtypes = [vp, vp]
    lib.srlhip_kuka_tree_default_model.argtypes = [vp]
    lib.srlhip_set_kuka_tree_model.argtypes = [vp, vp]
    lib.srlhip_render.argtypes = [vp, vp]
    lib.srlhip_stream.argtypes = [vp, ctypes.POINTER(vp)]
    lib.srlhip_copy_async.argtypes = [vp, vp, vp, ctypes.c_size_t]
    lib.srlhip_timing_end.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.srlhip_graph_begin.argtypes = [vp]
    lib.srlhip_graph_end.argtypes = [vp, ctypes.POINTER(vp)]
    lib.srlhip_graph_launch.argtypes = [vp, vp]
    lib.srlhip_graph_destroy.argtypes = [vp]
    lib.srlhip_encoder_supported.argtypes = [i32, i32, i32]
    lib.srlhip_encoder_feature_count.argtypes = [i32, i32, i32]
    lib.srlhip_encoder_feature_count.restype = i32
    lib.srlhip_encoder_create.argtypes = [i32, i32, i32, i32, i32] + [vp] * 8 + [ctypes.POINTER(vp)]
    lib.srlhip_encoder_forward.argtypes = [vp, vp, i32, vp, vp]
    lib.srlhip_encoder_overflow.argtypes = [vp, ctypes.POINTER(i32)]
    lib.srlhip_encoder_phase_cycles.argtypes = [vp, vp, i32, vp, vp]
    lib.srlhip_encoder_destroy.argtypes = [vp]
    lib.srlhip_encoder_last_error.restype = ctypes.c_char_p
    lib.srlhip_encoder_last_error.argtypes = [vp]
    lib.srlhip_pca_supported.argtypes = [ctypes.c_int64, i32]
    lib.srlhip_pca_create.argtypes = [i32, ctypes.c_int64, i32, vp, vp, ctypes.POINTER(vp)]
    lib.srlhip_pca_forward.argtypes = [vp, vp, i32, vp, i32, vp]
    lib.srlhip_pca_project_host.argtypes = [ctypes.c_int64, i32, vp, vp, vp, i32, vp, i32]
    lib.srlhip_pca_destroy.argtypes = [vp]
    lib.srlhip_pca_last_error.restype = ctypes.c_char_p
    lib.srlhip_pca_last_error.argtypes = [vp]
    lib.srlhip_pca_gram_supported.argtypes = [i32, ctypes.c_int64]
    lib.srlhip_pca_gram.argtypes = [i32, vp, i32, ctypes.c_int64, i32, vp, vp, vp]
    lib.srlhip_pca_gram_host.argtypes = [vp, i32, ctypes.c_int64, vp, vp]
    lib.srlhip_pca_gram_last_error.restype = ctypes.c_char_p
    lib.srlhip_pca_gram_last_error.argtypes = []
    lib.srlhip_knn_supported.argtypes = [i32] * 5
    lib.srlhip_knn_workspace_bytes.restype = ctypes.c_size_t
    lib.srlhip_knn_workspace_bytes.argtypes = [i32] * 5
    lib.srlhip_knn.argtypes = [i32, vp, i32, i32, i32, vp, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.srlhip_knn_host.argtypes = [vp, i32, i32, i32, vp, i32, i32, vp, i32, vp, vp, vp]
    lib.srlhip_knn_last_error.restype = ctypes.c_char_p
    lib.srlhip_knn_last_error.argtypes = []
    f64 = ctypes.c_double
    lib.srlhip_linear_srl_supported.argtypes = [ctypes.c_int64, i32, i32]
    lib.srlhip_linear_srl_workspace_bytes.restype = ctypes.c_size_t
    lib.srlhip_linear_srl_workspace_bytes.argtypes = [ctypes.c_int64, i32, i32]
    lib.srlhip_linear_srl_forward.argtypes = [i32, vp, i32, ctypes.c_int64, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    lib.srlhip_linear_srl_step.argtypes = [i32, vp, i32, ctypes.c_int64, i32, i32, vp, vp, vp, vp, vp, vp] + [f64] * 6 + [vp, vp]
    lib.srlhip_linear_srl_forward_host.argtypes = [vp, i32, ctypes.c_int64, i32, i32, vp, vp, vp, vp, vp]
    lib.srlhip_linear_srl_step_host.argtypes = [vp, i32, ctypes.c_int64, i32, i32, vp, vp, vp, vp, vp, vp] + [f64] * 6 + [vp]
    lib.srlhip_linear_srl_last_error.restype = ctypes.c_char_p
    lib.srlhip_linear_srl_last_error.argtypes = []
    lib.srlhip_encoder_pack_bytes.restype = ctypes.c_size_t
    lib.srlhip_encoder_pack_bytes.argtypes = []
    lib.srlhip_encoder_pack.argtypes = [vp, vp, vp, vp, vp, ctypes.c_size_t, vp]
    lib.srlhip_encoder_pack_i8_bytes.restype = ctypes.c_size_t
    lib.srlhip_encoder_pack_i8_bytes.argtypes = []
    lib.srlhip_encoder_pack_i8.argtypes = [vp, vp, i32, vp, ctypes.c_size_t, vp]
    lib.srlhip_encoder_pack_first_layer.argtypes = [i32, vp, vp, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_float)]
    lib.srlhip_jpeg_encode.argtypes = [i32, vp, i32, i32, i32, i32, i32, vp, ctypes.c_int64, vp, vp, vp]
    lib.srlhip_render_jpeg.argtypes = [vp, i32, vp, ctypes.c_int64, vp, vp]
    lib.srlhip_jpeg_header_bytes.restype = ctypes.c_size_t
    lib.srlhip_jpeg_header_bytes.argtypes = []
    lib.srlhip_jpeg_encode_host.argtypes = [vp, i32, i32, i32, i32, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]
    lib.srlhip_jpeg_probe.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.srlhip_jpeg_decode_host.argtypes = [vp, ctypes.c_size_t, vp, i32, ctypes.c_size_t, ctypes.POINTER(i32)]
    lib.srlhip_jpeg_decode_workspace_bytes.restype = ctypes.c_size_t
    lib.srlhip_jpeg_decode_workspace_bytes.argtypes = [i32, i32, i32]
    lib.srlhip_jpeg_decode.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.srlhip_jpeg_probe_baseline.argtypes = [vp, ctypes.c_size_t, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.srlhip_jpeg_decode_baseline_host.argtypes = [vp, ctypes.c_size_t, vp, i32, ctypes.c_size_t, ctypes.POINTER(i32)]
    lib.srlhip_jpeg_decode_baseline_workspace_bytes.restype = ctypes.c_size_t
    lib.srlhip_jpeg_decode_baseline_workspace_bytes.argtypes = [i32, i32, i32]
    lib.srlhip_jpeg_decode_baseline.argtypes = [i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    _lib = lib
    return lib


def default_config(env_kind):
    cfg = Config()
    rc = load().srlhip_default_config(env_kind, ctypes.byref(cfg))
    if rc:
        raise SrlHipError("srlhip_default_config({}) -> {}".format(env_kind, rc))
    return cfg


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, int):          # raw device pointer (io_device = 1)
        return ctypes.c_void_p(a)
    return a.ctypes.data_as(ctypes.c_void_p)


class Handle(object):
    """Thin object wrapper over srlhip_handle; numpy arrays in host-io mode,
    integer device pointers (e.g. torch.Tensor.data_ptr()) in device-io mode."""

    def __init__(self, cfg):
        self._lib = load()
        self._h = ctypes.c_void_p()
        self.cfg = cfg
        rc = self._lib.srlhip_create(ctypes.byref(cfg), ctypes.byref(self._h))
        if rc:
            self._h = None
            msg = self._lib.srlhip_last_error(None).decode()
            raise SrlHipError("srlhip_create failed ({}): {}".format(rc, msg))
        self.num_envs = cfg.num_envs
        self.obs_dim = self._lib.srlhip_obs_dim(self._h)
        self.obs_bytes = self._lib.srlhip_obs_bytes(self._h)
        self.action_dim = self._lib.srlhip_action_dim(self._h)
        self.num_actions = self._lib.srlhip_num_actions(self._h)
        self.reset_rand_count = self._lib.srlhip_reset_rand_count(self._h)
        # SRLHIP_KUKA_SDF=<.../pybullet_data/kuka_iiwa/kuka_with_gripper2.sdf>: take the arm model from the file the
        # reference loads (kuka.py:60) instead of the baked (recalled) table
        sdf = os.environ.get("SRLHIP_KUKA_SDF")
        if sdf and cfg.env_kind in (ENV_KUKA_BUTTON, ENV_KUKA_MOVING, ENV_KUKA_RAND):
            from . import kuka_model
            self.set_kuka_model(kuka_model.to_table(kuka_model.from_sdf(sdf)))

    def _check(self, rc, what):
        if rc:
            raise SrlHipError("{} failed ({}): {}".format(what, rc, self._lib.srlhip_last_error(self._h).decode()))

    def last_error(self):
        return self._lib.srlhip_last_error(self._h).decode()

    def close(self):
        if self._h:
            self._lib.srlhip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- allocation helpers (host io) -----------------------------------------
    def new_obs(self, T=None):
        n = self.num_envs
        lead = (n,) if T is None else (T, n)
        if self.cfg.obs_mode == OBS_RAW_PIXELS:
            ch = 6 if self.cfg.multi_view else 3
            return np.zeros(lead + (self.cfg.img_h, self.cfg.img_w, ch), np.uint8)
        return np.zeros(lead + (self.obs_dim,), np.float32)

    def action_array(self, actions, T=None):
        n = self.num_envs
        lead = (n,) if T is None else (T, n)
        if self.cfg.is_discrete:
            a = np.ascontiguousarray(actions, dtype=np.int32)
            assert a.shape == lead, (a.shape, lead)
        else:
            a = np.ascontiguousarray(none_rows(actions, self.action_dim, len(lead)), dtype=np.float32)
            assert a.shape == lead + (self.action_dim,), (a.shape, lead)
        return a

    # ---- ABI calls -------------------------------------------------------------
    def seed(self, seeds, mask=None):
        seeds = np.ascontiguousarray(seeds, dtype=np.int64)
        assert seeds.shape == (self.num_envs,)
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        self._check(self._lib.srlhip_seed(self._h, _ptr(m), _ptr(seeds)), "srlhip_seed")

    def reset(self, mask=None, host_rand=None, obs_out=None):
        m = None if mask is None else np.ascontiguousarray(mask, dtype=np.uint8)
        if host_rand is not None and not isinstance(host_rand, int):
            host_rand = np.ascontiguousarray(host_rand, dtype=np.float64)
            assert host_rand.shape == (self.num_envs, self.reset_rand_count)
        if obs_out is None and not self.cfg.io_device:
            obs_out = self.new_obs()
        self._check(self._lib.srlhip_reset(self._h, _ptr(m), _ptr(host_rand), _ptr(obs_out)), "srlhip_reset")
        return obs_out

    def step(self, actions, host_noise=None, out=None):
        if self.cfg.io_device:
            obs, rew, done = out
            self._check(self._lib.srlhip_step(self._h, _ptr(actions), _ptr(host_noise), _ptr(obs), _ptr(rew),
                                              _ptr(done)), "srlhip_step")
            return out
        a = self.action_array(actions)
        if host_noise is not None:
            host_noise = np.ascontiguousarray(host_noise, dtype=np.float64)
        if out is None:
            out = (self.new_obs(), np.zeros(self.num_envs, np.float32), np.zeros(self.num_envs, np.uint8))
        obs, rew, done = out
        self._check(self._lib.srlhip_step(self._h, _ptr(a), _ptr(host_noise), _ptr(obs), _ptr(rew), _ptr(done)),
                    "srlhip_step")
        return out

    def _new_planes(self, T, want, actions=True):
        """the host planes of a rollout call: (obs, reward, done, actions), a zeroed [T][N] array for every name in `want`, else None"""
        n = self.num_envs
        obs = self.new_obs(T) if "obs" in want else None
        rew = np.zeros((T, n), np.float32) if "reward" in want else None
        done = np.zeros((T, n), np.uint8) if "done" in want else None
        act = None
        if actions and "actions" in want:
            act = np.zeros((T, n), np.int32) if self.cfg.is_discrete else np.zeros((T, n, self.action_dim), np.float32)
        return obs, rew, done, act

    def rollout(self, T, actions=None, want=("obs", "reward", "done", "actions"), out=None):
        if self.cfg.io_device:
            obs, rew, done, act = out
            self._check(self._lib.srlhip_rollout(self._h, T, _ptr(actions), _ptr(obs), _ptr(rew), _ptr(done),
                                                 _ptr(act)), "srlhip_rollout")
            return out
        a = None if actions is None else self.action_array(actions, T)
        obs, rew, done, act = self._new_planes(T, want, actions=a is None)
        self._check(self._lib.srlhip_rollout(self._h, T, _ptr(a), _ptr(obs), _ptr(rew), _ptr(done), _ptr(act)),
                    "srlhip_rollout")
        return {"obs": obs, "reward": rew, "done": done, "actions": a if a is not None else act}

    def policy_shape(self, per_env=True):
        """shape of rollout_policy's weights: ([num_envs],) obs_dim, A with A = num_actions (discrete) or action_dim"""
        a = self.num_actions if self.cfg.is_discrete else self.action_dim
        return ((self.num_envs,) if per_env else ()) + (self.obs_dim, a)

    def _policy_struct(self, cls, per_env, freeze_after_done, obs_mean, obs_std, clip_obs):
        """a LinearPolicy / MlpPolicy with the fields the two structs share filled in (pointers: _rollout_policy_call)"""
        pol = cls()
        pol.struct_size, pol.per_env, pol.freeze_after_done = ctypes.sizeof(cls), int(bool(per_env)), int(bool(freeze_after_done))
        assert (obs_mean is None) == (obs_std is None), "obs_mean and obs_std come together"
        pol.normalize, pol.clip_obs = int(obs_mean is not None), float(clip_obs)
        return pol

    def _rollout_policy_call(self, name, T, pol, field, params, dtype, shape, obs_mean, obs_std, want, out):
        """the ABI call `name` with `pol`, whose parameter block is the struct field `field`: `params` as `dtype` of `shape` (None:
        unchecked) on a host-pointer handle, a raw device pointer on a device-pointer one"""
        fn = getattr(self._lib, name)
        if self.cfg.io_device:
            setattr(pol, field, params)
            pol.obs_mean, pol.obs_std = obs_mean, obs_std
            obs, rew, done, act = out
            self._check(fn(self._h, T, ctypes.byref(pol), _ptr(obs or None), _ptr(rew or None), _ptr(done or None),
                           _ptr(act or None)), name)
            return out
        w = np.ascontiguousarray(params, dtype=dtype)
        assert shape is None or w.shape == shape, (w.shape, shape)
        keep = [w]
        setattr(pol, field, w.ctypes.data)
        if obs_mean is not None:
            mean, std = np.ascontiguousarray(obs_mean, dtype=np.float64), np.ascontiguousarray(obs_std, dtype=np.float64)
            assert mean.shape == (self.obs_dim,) and std.shape == (self.obs_dim,), (mean.shape, std.shape)
            keep += [mean, std]
            pol.obs_mean, pol.obs_std = mean.ctypes.data, std.ctypes.data
        obs, rew, done, act = self._new_planes(T, want)
        self._check(fn(self._h, T, ctypes.byref(pol), _ptr(obs), _ptr(rew), _ptr(done), _ptr(act)), name)
        del keep
        return {"obs": obs, "reward": rew, "done": done, "actions": act}

    def rollout_policy(self, T, weights, per_env=True, freeze_after_done=False, obs_mean=None, obs_std=None, clip_obs=10.0,
                       want=("obs", "reward", "done", "actions"), out=None, sample=False):
        """srlhip_rollout_policy: T fused steps whose actions a linear policy picks inside the kernel from the env's own current
        observation (float64 scores; argmax with discrete actions, the float32 scores themselves with continuous ones).
        `weights`: float64 [num_envs][obs_dim][A] (per_env) or [obs_dim][A]; obs_mean / obs_std (float64 [obs_dim], both or
        neither): the observation is normalised and clipped to +-clip_obs first, with these statistics frozen for the call.
        Host-pointer handles take numpy arrays and return a dict of [T][N] planes (`want` selects them); device-pointer handles take
        raw device pointers for weights / mean / std and `out` = (obs, reward, done, actions) pointers (0 / None = skip).
        sample=True: srlhip_rollout_policy_sampled — discrete actions only, the action drawn from the softmax of the scores with the
        env's own action stream, ARS's default form (include/srlhip.h has the contract)."""
        pol = self._policy_struct(LinearPolicy, per_env, freeze_after_done, obs_mean, obs_std, clip_obs)
        return self._rollout_policy_call("srlhip_rollout_policy_sampled" if sample else "srlhip_rollout_policy", T, pol, "weights", weights, np.float64, self.policy_shape(per_env),
                                         obs_mean, obs_std, want, out)

    def mlp_param_count(self, hidden):
        """P of rollout_mlp_policy: H D + H + A H + A with D = obs_dim, A = num_actions (discrete) or action_dim"""
        a = self.num_actions if self.cfg.is_discrete else self.action_dim
        return hidden * self.obs_dim + hidden + a * hidden + a

    def rollout_mlp_policy(self, T, params, hidden, per_env=True, freeze_after_done=False, obs_mean=None, obs_std=None, clip_obs=10.0,
                           want=("obs", "reward", "done", "actions"), out=None, sample=False):
        """srlhip_rollout_mlp_policy: rollout_policy with a one-hidden-layer ReLU MLP as the score function.  `params`: float32
        [num_envs][P] (per_env) or [P], P = mlp_param_count(hidden), in nn.Module.parameters() order (fc_in.weight [H][D],
        fc_in.bias [H], fc_out.weight [A][H], fc_out.bias [A]) — a CMA-ES population as it is.  Everything else as rollout_policy
        (device-pointer handles: raw device pointers and `out`).  sample=True: srlhip_rollout_mlp_policy_sampled — discrete actions
        only, the action drawn from the softmax of the scores with the env's own action stream (include/srlhip.h has the contract)."""
        pol = self._policy_struct(MlpPolicy, per_env, freeze_after_done, obs_mean, obs_std, clip_obs)
        pol.hidden, pol.reserved = int(hidden), 0
        shape = None                                   # (hidden outside 1..128: the library refuses by name)
        if 1 <= int(hidden) <= 128:
            shape = ((self.num_envs,) if per_env else ()) + (self.mlp_param_count(int(hidden)),)
        return self._rollout_policy_call("srlhip_rollout_mlp_policy_sampled" if sample else "srlhip_rollout_mlp_policy", T, pol, "params", params, np.float32, shape,
                                         obs_mean, obs_std, want, out)

    def rollout_policy_summary(self, T, weights=None, params=None, hidden=None, sample=False, moments=True, per_env=True, freeze_after_done=False,
                               obs_mean=None, obs_std=None, clip_obs=10.0, out=None):
        """srlhip_rollout_policy_summary: rollout_policy (`weights`) or rollout_mlp_policy (`params` + `hidden`), with sample=True their
        sampled forms, returning what a learner keeps instead of the [T][N] planes: per env the return up to its first done of the
        call ("ret", float64 [N]), the live-step count ("length", int32 [N]) and, with `moments`, the sums of the live observations
        and of their squares ("obs_sum", "obs_sqsum", float64 [N][obs_dim]) — include/srlhip.h has the contract.  The env ends in the
        state the plane call leaves.  Host-pointer handles take numpy arrays and return a dict of new arrays; device-pointer handles
        take raw device pointers and `out` = (ret, length, obs_sum, obs_sqsum) pointers (0 / None = skip) and only enqueue."""
        assert (weights is None) != (params is None), "pass weights (linear policy) or params and hidden (MLP)"
        lin = mlp = None
        if params is None:
            pol = lin = self._policy_struct(LinearPolicy, per_env, freeze_after_done, obs_mean, obs_std, clip_obs)
            field, block, dtype, shape = "weights", weights, np.float64, self.policy_shape(per_env)
        else:
            pol = mlp = self._policy_struct(MlpPolicy, per_env, freeze_after_done, obs_mean, obs_std, clip_obs)
            pol.hidden, pol.reserved = int(hidden), 0
            field, block, dtype, shape = "params", params, np.float32, None      # (hidden outside 1..128: the library refuses by name)
            if 1 <= int(hidden) <= 128:
                shape = ((self.num_envs,) if per_env else ()) + (self.mlp_param_count(int(hidden)),)
        summ = RolloutSummary()
        summ.struct_size, summ.reserved = ctypes.sizeof(RolloutSummary), 0
        keep = []
        if self.cfg.io_device:
            setattr(pol, field, block)
            pol.obs_mean, pol.obs_std = obs_mean, obs_std
            summ.ret, summ.length, summ.obs_sum, summ.obs_sqsum = [p or None for p in out]
            result = out
        else:
            w = np.ascontiguousarray(block, dtype=dtype)
            assert shape is None or w.shape == shape, (w.shape, shape)
            keep.append(w)
            setattr(pol, field, w.ctypes.data)
            if obs_mean is not None:
                mean, std = np.ascontiguousarray(obs_mean, dtype=np.float64), np.ascontiguousarray(obs_std, dtype=np.float64)
                assert mean.shape == (self.obs_dim,) and std.shape == (self.obs_dim,), (mean.shape, std.shape)
                keep += [mean, std]
                pol.obs_mean, pol.obs_std = mean.ctypes.data, std.ctypes.data
            n = self.num_envs
            result = {"ret": np.zeros(n, np.float64), "length": np.zeros(n, np.int32)}
            if moments:
                result["obs_sum"], result["obs_sqsum"] = np.zeros((n, self.obs_dim), np.float64), np.zeros((n, self.obs_dim), np.float64)
            for k, a in result.items():
                setattr(summ, k, a.ctypes.data)
        self._check(self._lib.srlhip_rollout_policy_summary(self._h, T, None if lin is None else ctypes.byref(lin), None if mlp is None else ctypes.byref(mlp),
                                                            int(bool(sample)), ctypes.byref(summ)), "srlhip_rollout_policy_summary")
        del keep
        return result

    def policy_act(self, obs, obs_dim, act_out, weights=None, params=None, hidden=None, per_env=True, freeze_after_done=False,
                   obs_mean=None, obs_std=None, clip_obs=10.0, done_prev=None, frozen=None, sample=False, score_out=None):
        """srlhip_policy_act: one launch on the handle's stream that writes every env's action to `act_out` from the float32
        [num_envs][obs_dim] plane `obs` (include/srlhip.h has the order-exact contract).  Device-pointer handles only; every array
        argument is a raw device pointer.  `weights` (float64 [(num_envs)][obs_dim][A]): the linear policy; `params` + `hidden`
        (float32 [(num_envs)][P]): the MLP, sample=True draws its discrete action from the softmax with the env's action stream.
        done_prev: the done plane of the step that produced obs (None at the first step); frozen: uint8 [num_envs], needed with
        freeze_after_done; score_out: optional float64 [num_envs][A] plane for the scores.  Only enqueues: capturable between graph_begin / graph_end."""
        assert (weights is None) != (params is None), "pass weights (linear policy) or params and hidden (MLP)"
        lin = mlp = None
        if params is None:
            pol = lin = self._policy_struct(LinearPolicy, per_env, freeze_after_done, obs_mean, obs_std, clip_obs)
            pol.weights = weights
        else:
            pol = mlp = self._policy_struct(MlpPolicy, per_env, freeze_after_done, obs_mean, obs_std, clip_obs)
            pol.hidden, pol.reserved, pol.params = int(hidden), 0, params
        pol.obs_mean, pol.obs_std = obs_mean, obs_std
        self._check(self._lib.srlhip_policy_act(self._h, None if lin is None else ctypes.byref(lin), None if mlp is None else ctypes.byref(mlp),
                                                int(bool(sample)), _ptr(obs), int(obs_dim), _ptr(done_prev or None), _ptr(frozen or None),
                                                _ptr(act_out), _ptr(score_out or None)), "srlhip_policy_act")

    def cnn_param_count(self, A=None):
        """P of cnn_policy_act for this handle's frames: the reference's CNNPolicyPytorch (conv 5x5 to 8, 3x3 to 16, 3x3 to 32, each with
        batch-norm, then fc F -> A) in nn.Module.parameters() order; A defaults to num_actions (discrete) or action_dim"""
        if A is None:
            A = self.num_actions if self.cfg.is_discrete else self.action_dim
        p = int(self._lib.srlhip_cnn_param_count(6 if self.cfg.multi_view else 3, self.cfg.img_h, self.cfg.img_w, int(A)))
        if not p:
            raise SrlHipError("cnn_param_count: frames of {} x {} are outside the CNN policy's range (sides 43..224)".format(self.cfg.img_h, self.cfg.img_w))
        return p

    def cnn_policy_act(self, images, act_out, params, per_env=True, freeze_after_done=False, done_prev=None, frozen=None, sample=False,
                       score_out=None):
        """srlhip_cnn_policy_act: one launch on the handle's stream that writes every env's action to `act_out` from the uint8
        [num_envs][H][W][C] plane `images` that step / reset wrote, through the env's own CNN (include/srlhip.h has the contract).
        Device-pointer raw_pixels handles only; every array argument is a raw device pointer.  `params`: float32 [(num_envs)][P],
        P = cnn_param_count().  done_prev / frozen / sample as in policy_act; score_out: optional float32 [num_envs][A] plane.
        Only enqueues: capturable between graph_begin / graph_end."""
        pol = CnnPolicy()
        pol.struct_size, pol.per_env, pol.freeze_after_done, pol.reserved = ctypes.sizeof(CnnPolicy), int(bool(per_env)), int(bool(freeze_after_done)), 0
        pol.params = params
        self._check(self._lib.srlhip_cnn_policy_act(self._h, ctypes.byref(pol), int(bool(sample)), _ptr(images), _ptr(done_prev or None),
                                                    _ptr(frozen or None), _ptr(act_out), _ptr(score_out or None)), "srlhip_cnn_policy_act")

    def pixel_policy_act(self, images, act_out, weights, delta=None, noise=0.0, freeze_after_done=False, done_prev=None, frozen=None,
                         score_out=None):
        """srlhip_pixel_policy_act: one launch on the handle's stream that writes every env's action to `act_out` from the uint8
        [num_envs][H][W][C] plane `images` that step / reset wrote, through ARS's linear policy on the flattened frame (include/srlhip.h
        has the contract).  Device-pointer raw_pixels handles only; every array argument is a raw device pointer.  `weights`: float64
        M [D][A]; `delta`: float64 [num_envs / 2][D][A] — env 2k then acts with M + noise delta[k], env 2k + 1 with M - noise delta[k] —
        or None: every env acts with M.  done_prev / frozen as in policy_act; score_out: optional float64 [num_envs][A] plane.
        Only enqueues: capturable between graph_begin / graph_end."""
        pol = PixelPolicy()
        pol.struct_size, pol.paired, pol.freeze_after_done, pol.reserved = ctypes.sizeof(PixelPolicy), int(delta is not None), int(bool(freeze_after_done)), 0
        pol.weights, pol.delta, pol.noise = weights, delta, float(noise)
        self._check(self._lib.srlhip_pixel_policy_act(self._h, ctypes.byref(pol), _ptr(images), _ptr(done_prev or None), _ptr(frozen or None),
                                                      _ptr(act_out), _ptr(score_out or None)), "srlhip_pixel_policy_act")

    def sample_actions(self, scores, act_out, frozen=None):
        """srlhip_sample_actions: one launch on the handle's stream that draws every env's discrete action from the softmax of its row of
        the float64 [num_envs][A] plane `scores` (what policy_act / pixel_policy_act left in score_out) with the env's action stream, and
        moves that stream one block on.  frozen: optional uint8 [num_envs] plane, a frozen env gets -1.  Device-pointer handles only;
        every argument is a raw device pointer.  Only enqueues: capturable between graph_begin / graph_end."""
        self._check(self._lib.srlhip_sample_actions(self._h, _ptr(scores), _ptr(frozen or None), _ptr(act_out)), "srlhip_sample_actions")

    def get_state(self, field):
        dtype, k = _FIELD_SHAPES[field]
        out = np.zeros((k, self.num_envs) if k > 1 else (self.num_envs,), dtype)
        self._check(self._lib.srlhip_get_state(self._h, field, _ptr(out)), "srlhip_get_state")
        return out

    def set_state(self, field, value):
        dtype, k = _FIELD_SHAPES[field]
        v = np.ascontiguousarray(value, dtype=dtype)
        assert v.shape == ((k, self.num_envs) if k > 1 else (self.num_envs,))
        self._check(self._lib.srlhip_set_state(self._h, field, _ptr(v)), "srlhip_set_state")

    def device_ptr(self, field):
        p = ctypes.c_void_p()
        self._check(self._lib.srlhip_device_ptr(self._h, field, ctypes.byref(p)), "srlhip_device_ptr")
        return p.value

    def render(self, out=None):
        """uint8 [N][H][W][C] image of the current state of every env (tile rasteriser)."""
        if self.cfg.io_device:
            self._check(self._lib.srlhip_render(self._h, _ptr(out)), "srlhip_render")
            return out
        ch = 6 if self.cfg.multi_view else 3
        if out is None:
            out = np.zeros((self.num_envs, self.cfg.img_h, self.cfg.img_w, ch), np.uint8)
        self._check(self._lib.srlhip_render(self._h, _ptr(out)), "srlhip_render")
        return out

    def render_jpeg(self, quality=95, cap_per_stream=None):
        """srlhip_render_jpeg on a host-pointer handle: the current frame of every env as a baseline JPEG stream, encoded on the device
        -> list of bytes, num_envs of them (multi_view / fpv: 2 * num_envs, env i's two cameras at 2i and 2i + 1).  A stream larger
        than cap_per_stream (default 1024 + H * W * 3) comes back as None."""
        assert not self.cfg.io_device, "render_jpeg returns host bytes: device-pointer handles call srlhip_render_jpeg with their own buffers"
        ns = self.num_envs * (2 if self.cfg.multi_view else 1)
        cap = int(cap_per_stream) if cap_per_stream is not None else 1024 + self.cfg.img_h * self.cfg.img_w * 3
        blob, offsets, overflow = np.empty(ns * cap, np.uint8), np.zeros(ns + 1, np.int64), np.zeros(ns, np.int32)
        self._check(self._lib.srlhip_render_jpeg(self._h, int(quality), _ptr(blob), ctypes.c_int64(blob.nbytes), _ptr(offsets), _ptr(overflow)),
                    "srlhip_render_jpeg")
        return split_streams(blob, offsets, overflow)

    def set_kuka_model(self, table):
        """Install a runtime model table (srlhip_kuka_model: 138 float64, see srlhip.kuka_model) — reset() afterwards."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        assert t.shape == (KUKA_MODEL_DOUBLES,)
        self._check(self._lib.srlhip_set_kuka_model(self._h, _ptr(t)), "srlhip_set_kuka_model")

    def set_kuka_tree_model(self, table):
        """Install a full-model table (srlhip_kuka_tree_model: 510 float64) on a KUKA_MODEL_FULL handle — reset() afterwards."""
        t = np.ascontiguousarray(table, dtype=np.float64)
        assert t.shape == (KUKA_TREE_MODEL_DOUBLES,)
        self._check(self._lib.srlhip_set_kuka_tree_model(self._h, _ptr(t)), "srlhip_set_kuka_tree_model")

    def kuka_kernel(self):
        """'tree' (full model, 16 lanes per env), 'group' (lumped model, 16 lanes per env) or 'lane' (lumped, one lane per env):
        the kernel that steps this Kuka batch."""
        rc = self._lib.srlhip_kuka_kernel(self._h)
        if rc < 0:
            raise SrlHipError("srlhip_kuka_kernel: not a Kuka handle")
        return {0: "lane", 1: "group", 2: "tree"}[rc]

    def kuka_model_name(self):
        return "full 12-DoF gripper tree" if self.cfg.kuka_model == KUKA_MODEL_FULL else "lumped gripper (7 DoF)"

    def episode_stats_device(self, last_return=0, last_length=0, n_finished=0):
        """Enqueue-only: float32 returns / int32 lengths / counts of the last finished episodes into DEVICE buffers
        (raw pointers, 0 = skip) on the handle's stream."""
        self._check(self._lib.srlhip_episode_stats_device(self._h, last_return or None, last_length or None, n_finished or None),
                    "srlhip_episode_stats_device")

    def episode_records(self):
        """Zero-copy numpy views (last_return float64 [n], last_length int32 [n]) of the mapped host block a host-pointer handle's
        kernels write Monitor's (r, l) into: read entry i after a step / rollout call in which env i reported done."""
        r, l = ctypes.c_void_p(), ctypes.c_void_p()
        self._check(self._lib.srlhip_episode_records(self._h, ctypes.byref(r), ctypes.byref(l)), "srlhip_episode_records")
        n = self.num_envs
        ret = np.ctypeslib.as_array(ctypes.cast(r, ctypes.POINTER(ctypes.c_double)), shape=(n,))
        length = np.ctypeslib.as_array(ctypes.cast(l, ctypes.POINTER(ctypes.c_int32)), shape=(n,))
        ret.flags.writeable = length.flags.writeable = False
        return ret, length

    def step_fn(self, actions, host_noise=None):
        """A closure for per-step loops on a host-pointer handle: the output arrays, their ctypes pointers and the C entry point are
        bound once, so a step costs one foreign call.  `actions` is the caller's int32 / float32 array that it refills in place
        before every call; returns (call, obs, reward, done) — call() steps and returns the library's status code."""
        assert not self.cfg.io_device
        a = self.action_array(actions)
        assert a is actions, "step_fn needs the final contiguous int32 / float32 action array"
        obs, rew, done = self.new_obs(), np.zeros(self.num_envs, np.float32), np.zeros(self.num_envs, np.uint8)
        fn, hh = self._lib.srlhip_step, self._h
        pa, pn, po, pr, pd = _ptr(a), _ptr(host_noise), _ptr(obs), _ptr(rew), _ptr(done)
        return (lambda: fn(hh, pa, pn, po, pr, pd)), obs, rew, done

    def step_split_fn(self, actions, obs, rew, done):
        """The two halves of a per-step loop on a host-pointer handle, bound once to the CALLER's arrays (contiguous, e.g. this
        shard's slices of global planes): go() = srlhip_step_async on `actions` (refilled in place before every call), collect() =
        srlhip_step_wait into obs / rew / done.  Both return the library's status code."""
        assert not self.cfg.io_device
        assert self.action_array(actions) is actions, "step_split_fn needs the final contiguous int32 / float32 action array"
        assert obs.flags.c_contiguous and obs.nbytes == self.obs_bytes * self.num_envs, (obs.shape, obs.dtype)
        assert rew.flags.c_contiguous and rew.dtype == np.float32 and rew.shape == (self.num_envs,)
        assert done.flags.c_contiguous and done.dtype == np.uint8 and done.shape == (self.num_envs,)
        go, wait, hh = self._lib.srlhip_step_async, self._lib.srlhip_step_wait, self._h
        pa, po, pr, pd = _ptr(actions), _ptr(obs), _ptr(rew), _ptr(done)
        keep = (actions, obs, rew, done)                     # the pointers above borrow these arrays
        return (lambda: go(hh, pa, None)), (lambda _keep=keep: wait(hh, po, pr, pd))

    def step_async(self, actions, host_noise=None):
        """srlhip_step_async: enqueue one step of a host-pointer handle (returns before the GPU has run it)"""
        a = self.action_array(actions)
        if host_noise is not None:
            host_noise = np.ascontiguousarray(host_noise, dtype=np.float64)
        self._check(self._lib.srlhip_step_async(self._h, _ptr(a), _ptr(host_noise)), "srlhip_step_async")

    def step_wait(self, out=None):
        """srlhip_step_wait: (obs, reward, done) of the step srlhip_step_async enqueued"""
        if out is None:
            out = (self.new_obs(), np.zeros(self.num_envs, np.float32), np.zeros(self.num_envs, np.uint8))
        obs, rew, done = out
        self._check(self._lib.srlhip_step_wait(self._h, _ptr(obs), _ptr(rew), _ptr(done)), "srlhip_step_wait")
        return out

    def step_pending(self):
        return self._lib.srlhip_step_pending(self._h) == 1

    def set_persistent(self, on=True, park_us=0):
        """srlhip_set_persistent: per-step calls without a launch per step (a resident kernel takes its steps through mapped memory).
        Raises SrlHipError (ENOTSUP) for handles that have no persistent form."""
        self._check(self._lib.srlhip_set_persistent(self._h, int(bool(on)), int(park_us)), "srlhip_set_persistent")

    def episode_stats(self):
        n = self.num_envs
        ret, length, fin = np.zeros(n, np.float64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self._check(self._lib.srlhip_episode_stats(self._h, _ptr(ret), _ptr(length), _ptr(fin)),
                    "srlhip_episode_stats")
        return ret, length, fin

    def sync(self):
        self._check(self._lib.srlhip_sync(self._h), "srlhip_sync")

    def copy_async(self, dst, src, nbytes):
        """srlhip_copy_async: raw pointers (device, or pinned host), enqueued on the handle's stream"""
        self._check(self._lib.srlhip_copy_async(self._h, ctypes.c_void_p(dst), ctypes.c_void_p(src), ctypes.c_size_t(nbytes)), "srlhip_copy_async")

    def stream(self):
        p = ctypes.c_void_p()
        self._check(self._lib.srlhip_stream(self._h, ctypes.byref(p)), "srlhip_stream")
        return p.value

    # ---- HIP graphs (device-io handles): capture a step sequence once, replay it with one launch per step
    def graph_begin(self):
        self._check(self._lib.srlhip_graph_begin(self._h), "srlhip_graph_begin")

    def graph_end(self):
        g = ctypes.c_void_p()
        self._check(self._lib.srlhip_graph_end(self._h, ctypes.byref(g)), "srlhip_graph_end")
        return g

    def graph_launch(self, g):
        self._check(self._lib.srlhip_graph_launch(self._h, g), "srlhip_graph_launch")

    def graph_destroy(self, g):
        self._lib.srlhip_graph_destroy(g)

    def timing_begin(self):
        self._check(self._lib.srlhip_timing_begin(self._h), "srlhip_timing_begin")

    def timing_end(self):
        ms = ctypes.c_float()
        self._check(self._lib.srlhip_timing_end(self._h, ctypes.byref(ms)), "srlhip_timing_end")
        return ms.value


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def none_rows(actions, dim, lead_ndim=1):
    """Continuous actions that may hold the reference's `None` -> float32 [..., dim] with a row of NaNs for every `None` (include/srlhip.h:
    a Kuka env's `None`; MobileRobot handles refuse it).  `lead_ndim` leading axes ([N]: 1, [T][N]: 2).  A numeric ndarray passes as
    it is (NaN rows included): only lists and object arrays are scanned."""
    if isinstance(actions, np.ndarray) and actions.dtype != object:
        return np.asarray(actions, dtype=np.float32)
    nan_row = np.full(dim, np.nan, np.float32)

    def rows(x, depth):
        if depth == 0:
            return nan_row if x is None else np.asarray(x, dtype=np.float32).reshape(dim)
        return np.stack([rows(y, depth - 1) for y in x]) if len(x) else np.zeros((0, dim), np.float32)
    return rows(actions, lead_ndim)


def split_streams(blob, offsets, overflow):
    """(blob, offsets [ns + 1], overflow [ns]) of srlhip_jpeg_encode / srlhip_render_jpeg as host arrays -> list of bytes, None where a stream overflowed"""
    return [None if overflow[s] else blob[offsets[s]:offsets[s + 1]].tobytes() for s in range(len(overflow))]


def jpeg_header_bytes():
    return int(load().srlhip_jpeg_header_bytes())


def jpeg_encode(images_dev_ptr, n, h, w, c, quality, blob_dev_ptr, cap_per_stream, offsets_dev_ptr, overflow_dev_ptr, device_id=0, stream=0):
    """srlhip_jpeg_encode, raw: device pointers (uint8 [n][h][w][c] frames in; blob of n * c / 3 * cap_per_stream bytes, int64 offsets
    [n * c / 3 + 1], int32 overflow [n * c / 3] out); only enqueues on `stream`.  Returns the library's status code."""
    return load().srlhip_jpeg_encode(int(device_id), _ptr(images_dev_ptr), int(n), int(h), int(w), int(c), int(quality), _ptr(blob_dev_ptr),
                                     ctypes.c_int64(cap_per_stream), _ptr(offsets_dev_ptr), _ptr(overflow_dev_ptr),
                                     ctypes.c_void_p(stream) if stream else None)


def jpeg_encode_host(frame, quality, cap=None):
    """srlhip_jpeg_encode_host: one uint8 [h][w][3] frame (any pixel stride: a 3-channel view of a 6-channel frame passes as it is)
    through the kernels' own source on the CPU -> bytes; raises SrlHipError on a refusal."""
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 3 and frame.shape[2] == 3 and frame.strides[2] == 1
    h, w = frame.shape[:2]
    assert frame.strides[0] == w * frame.strides[1], "rows must follow each other without padding"
    cap = int(cap) if cap is not None else 1024 + 4 * h * w * 3
    out, n = np.zeros(cap, np.uint8), ctypes.c_size_t(0)
    rc = load().srlhip_jpeg_encode_host(ctypes.c_void_p(frame.ctypes.data), h, w, int(frame.strides[1]), int(quality), _ptr(out), cap, ctypes.byref(n))
    if rc:
        raise SrlHipError("srlhip_jpeg_encode_host failed ({}), stream size {}".format(rc, n.value))
    return out[:n.value].tobytes()


JPEG_OK, JPEG_BAD_HEADER, JPEG_EMPTY, JPEG_BAD_DATA = 0, 1, 2, 3          # status_dev of srlhip_jpeg_decode


def jpeg_probe(data):
    """srlhip_jpeg_probe: (h, w) when `data` (bytes) has the layout the library's encoder writes, else None; no GPU needed"""
    buf = np.frombuffer(bytes(data), np.uint8)
    h, w = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = load().srlhip_jpeg_probe(ctypes.c_void_p(buf.ctypes.data if len(buf) else None), len(buf), ctypes.byref(h), ctypes.byref(w))
    return (int(h.value), int(w.value)) if rc == 0 else None


def jpeg_decode_host(data, out=None, return_status=False):
    """srlhip_jpeg_decode_host: one stream through the kernels' own source on the CPU -> uint8 [h][w][3].  `out`: a uint8 [h][w][3] view
    to write into (any pixel stride: channels 0..2 or 3..5 of a 6-channel frame).  Raises ValueError when the stream is not in the
    accepted format, SrlHipError when its data is malformed — or, with return_status, returns (frame, status) for statuses 0 and 3."""
    buf = np.frombuffer(bytes(data), np.uint8)
    hw = jpeg_probe(data)
    if hw is None:
        raise ValueError("not a stream of the library's encoder")
    h, w = hw
    if out is None:
        out = np.zeros((h, w, 3), np.uint8)
    assert out.dtype == np.uint8 and out.shape == (h, w, 3) and out.strides[2] == 1 and out.strides[0] == w * out.strides[1]
    stride = int(out.strides[1])
    status = ctypes.c_int32(-1)
    rc = load().srlhip_jpeg_decode_host(ctypes.c_void_p(buf.ctypes.data), len(buf), ctypes.c_void_p(out.ctypes.data), stride,
                                        (h * w - 1) * stride + 3, ctypes.byref(status))
    if rc:
        raise SrlHipError("srlhip_jpeg_decode_host failed ({})".format(rc))
    if return_status:
        return out, int(status.value)
    if status.value:
        raise SrlHipError("srlhip_jpeg_decode_host: malformed entropy-coded data (status {})".format(status.value))
    return out


def jpeg_decode_workspace_bytes(n_streams, h, w):
    return int(load().srlhip_jpeg_decode_workspace_bytes(int(n_streams), int(h), int(w)))


def jpeg_decode(blob_dev_ptr, offsets_dev_ptr, n_streams, h, w, c, images_dev_ptr, status_dev_ptr, workspace_dev_ptr, device_id=0, stream=0):
    """srlhip_jpeg_decode, raw: device pointers (the blob and int64 offsets [n_streams + 1] of srlhip_jpeg_encode in; uint8
    [n_streams * 3 / c][h][w][c] frames and int32 status [n_streams] out; jpeg_decode_workspace_bytes of scratch); only enqueues on
    `stream`.  Returns the library's status code."""
    return load().srlhip_jpeg_decode(int(device_id), _ptr(blob_dev_ptr), _ptr(offsets_dev_ptr), int(n_streams), int(h), int(w), int(c),
                                     _ptr(images_dev_ptr), _ptr(status_dev_ptr), _ptr(workspace_dev_ptr),
                                     ctypes.c_void_p(stream) if stream else None)


def jpeg_probe_baseline(data):
    """srlhip_jpeg_probe_baseline: (h, w, sampling) with sampling 420 or 444 when `data` (bytes) is a baseline stream of the accepted
    layout (what libjpeg writes by default, the library's own streams included), else None; no GPU needed"""
    buf = np.frombuffer(bytes(data), np.uint8)
    h, w, mode = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    rc = load().srlhip_jpeg_probe_baseline(ctypes.c_void_p(buf.ctypes.data if len(buf) else None), len(buf), ctypes.byref(h), ctypes.byref(w),
                                           ctypes.byref(mode))
    return (int(h.value), int(w.value), int(mode.value)) if rc == 0 else None


def jpeg_decode_baseline_host(data, out=None, return_status=False, shape=None):
    """srlhip_jpeg_decode_baseline_host: one stream through the kernels' own source on the CPU -> uint8 [h][w][3]; `out` and the errors
    as jpeg_decode_host.  With `shape` = (h, w) the stream is decoded as a device call for these sides would: a header that is refused
    or carries other sides gives a frame of zeros and status 1 (2 for an empty stream), returned with return_status, raised without."""
    buf = np.frombuffer(bytes(data), np.uint8)
    probed = jpeg_probe_baseline(data)
    if probed is None or (shape is not None and tuple(shape) != probed[:2]):
        if shape is None or not return_status:
            raise ValueError("not a baseline stream of the accepted layout" + ("" if shape is None else " for {}x{} frames".format(*shape)))
        if out is None:
            out = np.zeros(tuple(shape) + (3,), np.uint8)
        out[...] = 0
        return out, (JPEG_EMPTY if len(buf) == 0 else JPEG_BAD_HEADER)
    h, w = probed[:2]
    if out is None:
        out = np.zeros((h, w, 3), np.uint8)
    assert out.dtype == np.uint8 and out.shape == (h, w, 3) and out.strides[2] == 1 and out.strides[0] == w * out.strides[1]
    stride = int(out.strides[1])
    status = ctypes.c_int32(-1)
    rc = load().srlhip_jpeg_decode_baseline_host(ctypes.c_void_p(buf.ctypes.data), len(buf), ctypes.c_void_p(out.ctypes.data), stride,
                                                 (h * w - 1) * stride + 3, ctypes.byref(status))
    if rc:
        raise SrlHipError("srlhip_jpeg_decode_baseline_host failed ({})".format(rc))
    if return_status:
        return out, int(status.value)
    if status.value:
        raise SrlHipError("srlhip_jpeg_decode_baseline_host: malformed entropy-coded data (status {})".format(status.value))
    return out


def jpeg_decode_baseline_workspace_bytes(n_streams, h, w):
    return int(load().srlhip_jpeg_decode_baseline_workspace_bytes(int(n_streams), int(h), int(w)))


def jpeg_decode_baseline(blob_dev_ptr, offsets_dev_ptr, n_streams, h, w, c, images_dev_ptr, status_dev_ptr, workspace_dev_ptr, device_id=0, stream=0):
    """srlhip_jpeg_decode_baseline, raw: device pointers as jpeg_decode's, jpeg_decode_baseline_workspace_bytes of scratch; only enqueues
    on `stream`.  Returns the library's status code."""
    return load().srlhip_jpeg_decode_baseline(int(device_id), _ptr(blob_dev_ptr), _ptr(offsets_dev_ptr), int(n_streams), int(h), int(w), int(c),
                                              _ptr(images_dev_ptr), _ptr(status_dev_ptr), _ptr(workspace_dev_ptr),
                                              ctypes.c_void_p(stream) if stream else None)


def encoder_supported(img_h, img_w, n_channels):
    return bool(load().srlhip_encoder_supported(int(img_h), int(img_w), int(n_channels)))


def encoder_pack_first_layer(conv1_w, conv1_b):
    """Host-only: (layer 1's packed MFMA B-operand image of the layered encoder as float16 words, its power-of-two pre-scale)
    for 3- or 6-channel frames — csrc/encoder_general.hip's packer, as srlhip_encoder_create uploads it."""
    lib = load()
    w1, b1 = _f32(conv1_w), _f32(conv1_b)
    c = w1.shape[1]
    assert w1.shape == (64, c, 7, 7) and c in (3, 6) and b1.shape == (64,)
    out = np.zeros(2 * (14 if c == 3 else 28) * 1024, np.float16)
    scale = ctypes.c_float()
    rc = lib.srlhip_encoder_pack_first_layer(c, _ptr(w1), _ptr(b1), _ptr(out), ctypes.c_size_t(out.nbytes), ctypes.byref(scale))
    if rc:
        raise SrlHipError("srlhip_encoder_pack_first_layer failed ({})".format(rc))
    return out, float(scale.value)


def encoder_feature_count(img_h, img_w, n_channels):
    """inputs of the encoder's fully connected layer for this frame shape, 0 when the shape is not covered"""
    return int(load().srlhip_encoder_feature_count(int(img_h), int(img_w), int(n_channels)))


def encoder_pack(conv1_w, conv1_b, conv2_w, conv3_w):
    """Host-only: (packed MFMA B-operand image as float16 words, the three per-layer power-of-two weight scales)
    exactly as srlhip_encoder_create uploads them."""
    lib = load()
    out = np.zeros(lib.srlhip_encoder_pack_bytes() // 2, np.float16)
    w1, b1, w2, w3 = _f32(conv1_w), _f32(conv1_b), _f32(conv2_w), _f32(conv3_w)
    assert w1.shape == (64, 3, 7, 7) and b1.shape == (64,) and w2.shape == (64, 64, 3, 3) and w3.shape == (64, 64, 3, 3)
    scales = np.zeros(3, np.float32)
    rc = lib.srlhip_encoder_pack(_ptr(w1), _ptr(b1), _ptr(w2), _ptr(w3), _ptr(out), out.nbytes, _ptr(scales))
    if rc:
        raise SrlHipError("srlhip_encoder_pack failed ({})".format(rc))
    return out, scales


def encoder_pack_i8(conv1_w, conv1_b, zero_slot=0):
    """Host-only: (int8 digits [2][7][3][64][16], float32 [64] per-channel 256 / scale) of the int8 layer 1 — zero_slot 0: the fused
    64x64x3 kernel's layout, 7: the layered kernels' (3-channel frames of any other size)."""
    lib = load()
    w1, b1 = _f32(conv1_w), _f32(conv1_b)
    assert w1.shape == (64, 3, 7, 7) and b1.shape == (64,)
    out = np.zeros(lib.srlhip_encoder_pack_i8_bytes(), np.int8)
    inv = np.zeros(64, np.float32)
    rc = lib.srlhip_encoder_pack_i8(_ptr(w1), _ptr(b1), int(zero_slot), _ptr(out), out.nbytes, _ptr(inv))
    if rc:
        raise SrlHipError("srlhip_encoder_pack_i8 failed ({})".format(rc))
    return out.reshape(2, 7, 3, 64, 16), inv


class Encoder(object):
    """srlhip_encoder_handle: the CustomCNN forward on device-resident uint8 frames — one fused kernel for 64x64x3
    (csrc/encoder.hip), the layered kernels of csrc/encoder_general.hip for any other shape.
    Weights: float32 arrays in torch layout with the BatchNorms already folded (see include/srlhip.h); fc_w is
    [state_dim][64 * pooled cells] in torch's flatten order."""

    def __init__(self, device_id, img_shape, n_channels, state_dim, conv1, conv2, conv3, fc):
        self._lib = load()
        self._e = ctypes.c_void_p()
        arrs = [_f32(a) for pair in (conv1, conv2, conv3, fc) for a in pair]
        assert arrs[0].shape == (64, n_channels, 7, 7) and arrs[2].shape == (64, 64, 3, 3) and arrs[4].shape == (64, 64, 3, 3)
        assert arrs[6].shape == (state_dim, encoder_feature_count(img_shape[0], img_shape[1], n_channels)) and arrs[7].shape == (state_dim,)
        rc = self._lib.srlhip_encoder_create(int(device_id), int(img_shape[0]), int(img_shape[1]), int(n_channels),
                                             int(state_dim), *[_ptr(a) for a in arrs], ctypes.byref(self._e))
        if rc:
            self._e = None
            raise SrlHipError("srlhip_encoder_create failed ({}): {}".format(
                rc, self._lib.srlhip_encoder_last_error(None).decode()))
        self.state_dim = int(state_dim)

    def _check(self, rc, what):
        if rc:
            raise SrlHipError("{} failed ({}): {}".format(what, rc, self._lib.srlhip_encoder_last_error(self._e).decode()))

    def forward(self, images_ptr, n, states_ptr, stream=None):
        """images_ptr / states_ptr: raw device pointers (e.g. torch.Tensor.data_ptr()); enqueue-only on `stream`."""
        self._check(self._lib.srlhip_encoder_forward(self._e, _ptr(images_ptr), int(n), _ptr(states_ptr),
                                                     ctypes.c_void_p(stream) if stream else None), "srlhip_encoder_forward")

    PHASES = ("unpack", "layer1", "barrier1", "layer2_kloop", "layer2_epilogue", "barrier2", "layer3", "fc", "turnaround")

    def phase_cycles(self, images_ptr, n, states_ptr):
        """Diagnostic forward: {phase: shader cycles} of workgroup 0 (slowest wave, averaged over its first frames)."""
        c = np.zeros(9, np.int64)
        self._check(self._lib.srlhip_encoder_phase_cycles(self._e, _ptr(images_ptr), int(n), _ptr(states_ptr), _ptr(c)),
                    "srlhip_encoder_phase_cycles")
        return dict(zip(self.PHASES, c.tolist()))

    def overflow(self):
        flag = ctypes.c_int32()
        self._check(self._lib.srlhip_encoder_overflow(self._e, ctypes.byref(flag)), "srlhip_encoder_overflow")
        return bool(flag.value)

    def close(self):
        if self._e:
            self._lib.srlhip_encoder_destroy(self._e)
            self._e = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pca_supported(n_features, state_dim):
    """host only: does srlhip_pca_create take this shape (1 <= state_dim <= 64, n_features >= 1)"""
    return bool(load().srlhip_pca_supported(int(n_features), int(state_dim)))


def _pca_weights(w, b):
    w, b = np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert w.ndim == 2 and b.shape == (w.shape[1],), (w.shape, b.shape)
    return w, b


def pca_project_host(w, b, images, states_f32=False):
    """srlhip_pca_project_host: the kernel's own arithmetic (csrc/pca_project.hpp) on the CPU.  w float64 [F][S], b [S], images uint8
    [n][...] (flattened to [n][F]) -> float64 (states_f32: float32) [n][S]; raises SrlHipError on a refusal."""
    w, b = _pca_weights(w, b)
    images = np.ascontiguousarray(images, dtype=np.uint8)
    n = images.shape[0]
    images = images.reshape(n, w.shape[0])
    out = np.zeros((n, w.shape[1]), np.float32 if states_f32 else np.float64)
    rc = load().srlhip_pca_project_host(w.shape[0], w.shape[1], _ptr(w), _ptr(b), _ptr(images), n, _ptr(out), int(bool(states_f32)))
    if rc:
        raise SrlHipError("srlhip_pca_project_host failed ({})".format(rc))
    return out


class PcaProjector(object):
    """srlhip_pca_handle: the PCA state baseline on device-resident uint8 frames, one launch (csrc/pca_project.hip).
    w: float64 [n_features][state_dim] (whitened, transposed), b: float64 [state_dim] = -(mean_ @ w) — see include/srlhip.h."""

    def __init__(self, device_id, w, b):
        self._lib = load()
        self._p = ctypes.c_void_p()
        w, b = _pca_weights(w, b)
        rc = self._lib.srlhip_pca_create(int(device_id), w.shape[0], w.shape[1], _ptr(w), _ptr(b), ctypes.byref(self._p))
        if rc:
            self._p = None
            raise SrlHipError("srlhip_pca_create failed ({}): {}".format(rc, self._lib.srlhip_pca_last_error(None).decode()))
        self.n_features, self.state_dim = int(w.shape[0]), int(w.shape[1])

    def forward(self, images_ptr, n, states_ptr, states_f32=False, stream=None):
        """images_ptr / states_ptr: raw device pointers (e.g. torch.Tensor.data_ptr()); states float64 [n][state_dim], or float32 with
        states_f32; enqueue-only on `stream`."""
        rc = self._lib.srlhip_pca_forward(self._p, _ptr(images_ptr), int(n), _ptr(states_ptr), int(bool(states_f32)),
                                          ctypes.c_void_p(stream) if stream else None)
        if rc:
            raise SrlHipError("srlhip_pca_forward failed ({}): {}".format(rc, self._lib.srlhip_pca_last_error(self._p).decode()))

    def close(self):
        if self._p:
            self._lib.srlhip_pca_destroy(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


GRAM_MAX_FRAMES, GRAM_CHUNK = 8192, 65536


def pca_gram_supported(n, n_features):
    """host only: does srlhip_pca_gram take this shape (1 <= n <= 8192, n_features >= 1, 2 n^2 n_features 65025 < 2^63)"""
    return bool(load().srlhip_pca_gram_supported(int(n), int(n_features)))


def _gram_fail(what, rc):
    raise SrlHipError("{} failed ({}): {}".format(what, rc, load().srlhip_pca_gram_last_error().decode()))


def pca_gram(device_id, frames_ptr, n, n_features, gram_ptr, rowsum_ptr, split=0, stream=None):
    """srlhip_pca_gram: gram int64 [n][n] = X X^T and rowsum int64 [n] of the device-resident uint8 frames [n][n_features], exactly
    (csrc/pca_gram.hip).  Raw device pointers (e.g. torch.Tensor.data_ptr()); enqueue-only on `stream`; split 0 = automatic."""
    rc = load().srlhip_pca_gram(int(device_id), _ptr(frames_ptr), int(n), int(n_features), int(split), _ptr(gram_ptr), _ptr(rowsum_ptr),
                                ctypes.c_void_p(stream) if stream else None)
    if rc:
        _gram_fail("srlhip_pca_gram", rc)


def pca_gram_host(frames):
    """srlhip_pca_gram_host: the same two planes on the CPU, plain int64 loops.  frames uint8 [n][...] (flattened to [n][F]) ->
    (gram int64 [n][n], rowsum int64 [n]); raises SrlHipError on a refusal."""
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n = frames.shape[0]
    frames = frames.reshape(n, int(np.prod(frames.shape[1:])))
    gram, rowsum = np.zeros((n, n), np.int64), np.zeros(n, np.int64)
    rc = load().srlhip_pca_gram_host(_ptr(frames), n, frames.shape[1], _ptr(gram), _ptr(rowsum))
    if rc:
        _gram_fail("srlhip_pca_gram_host", rc)
    return gram, rowsum


KNN_MAX_N, KNN_MAX_S, KNN_MAX_K, KNN_MAX_G = 1 << 20, 64, 32, 32


def knn_supported(n, s, k, q, g=0):
    """host only: does srlhip_knn take this shape (2 <= n <= 2^20, 1 <= s <= 64, 1 <= k <= min(32, n - 1), 1 <= q <= 2^20, g = 0 for no
    ground truth or 1..32)"""
    return bool(load().srlhip_knn_supported(int(n), int(s), int(k), int(q), int(g)))


def knn_workspace_bytes(n, s, k, q, split=0):
    """bytes of device workspace srlhip_knn needs for this shape and split (0: the shape is refused)"""
    return int(load().srlhip_knn_workspace_bytes(int(n), int(s), int(k), int(q), int(split)))


def _knn_fail(what, rc):
    raise SrlHipError("{} failed ({}): {}".format(what, rc, load().srlhip_knn_last_error().decode()))


def knn(device_id, states_ptr, states_f32, n, s, queries_ptr, q, k, gt_ptr, g, idx_ptr, dist_ptr, err_ptr, workspace_ptr, split=0, stream=None):
    """srlhip_knn: idx int32 [q][k] and dist float64 [q][k], the exact k nearest neighbours of the query rows among the device-resident
    states [n][s] (float64, or float32 with states_f32), and with a ground truth [n][g] err float64 [q] (csrc/knn.hip; the contract is in
    include/srlhip.h).  Raw device pointers (e.g. torch.Tensor.data_ptr()), None for queries (every row), ground truth and err;
    workspace of knn_workspace_bytes; enqueue-only on `stream`; split 0 = automatic."""
    rc = load().srlhip_knn(int(device_id), _ptr(states_ptr), int(bool(states_f32)), int(n), int(s), _ptr(queries_ptr), int(q), int(k),
                           _ptr(gt_ptr), int(g), int(split), _ptr(idx_ptr), _ptr(dist_ptr), _ptr(err_ptr), _ptr(workspace_ptr),
                           ctypes.c_void_p(stream) if stream else None)
    if rc:
        _knn_fail("srlhip_knn", rc)


def knn_host(states, k, queries=None, ground_truth=None):
    """srlhip_knn_host: the same planes on the CPU.  states float64 or float32 [n][s], queries int32 [q] or None (every row),
    ground_truth float64 [n][g] or None -> (idx int32 [q][k], dist float64 [q][k][, err float64 [q]]); raises SrlHipError on a refusal."""
    states = np.asarray(states)
    states = np.ascontiguousarray(states, dtype=np.float32 if states.dtype == np.float32 else np.float64)
    if states.ndim != 2:
        raise ValueError("knn_host takes states [n][s]")
    n, s = states.shape
    if queries is not None:
        queries = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
    q = n if queries is None else len(queries)
    g = 0
    if ground_truth is not None:
        ground_truth = np.ascontiguousarray(ground_truth, dtype=np.float64)
        if ground_truth.ndim != 2 or ground_truth.shape[0] != n:
            raise ValueError("knn_host takes ground_truth [n][g]")
        g = ground_truth.shape[1]
    k = int(k)
    idx, dist = np.zeros((q, max(k, 0)), np.int32), np.zeros((q, max(k, 0)), np.float64)
    err = np.zeros(q, np.float64) if ground_truth is not None else None
    rc = load().srlhip_knn_host(_ptr(states), int(states.dtype == np.float32), n, s, _ptr(queries), q, k, _ptr(ground_truth), g,
                                _ptr(idx), _ptr(dist), _ptr(err))
    if rc:
        _knn_fail("srlhip_knn_host", rc)
    return (idx, dist) if err is None else (idx, dist, err)


# ---- the trainable linear state encoder (csrc/linear_srl.hip; the contract is in include/srlhip.h) ---------------------------------------
LINEAR_SRL_MAX_FRAMES = 1024


def linear_srl_supported(n_features, state_dim, n_channels=3):
    """host only: does srlhip_linear_srl_* take this shape (n_features >= 1, 1 <= state_dim <= 64, 1 <= n_channels <= 8)"""
    return bool(load().srlhip_linear_srl_supported(int(n_features), int(state_dim), int(n_channels)))


def linear_srl_workspace_bytes(n_features, state_dim, n):
    """bytes of device workspace srlhip_linear_srl_forward needs (0: the shape is refused)"""
    return int(load().srlhip_linear_srl_workspace_bytes(int(n_features), int(state_dim), int(n)))


def linear_srl_tables(n_channels, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225)):
    """-> (scale, offset) float64 [n_channels]: 1 / (255 std) and mean / std of the channel's ImageNet constant, repeated per 3-channel
    group (state_representation.models.preprocess)"""
    mean = np.array([mean[k % len(mean)] for k in range(n_channels)], np.float64)
    std = np.array([std[k % len(std)] for k in range(n_channels)], np.float64)
    return 1.0 / (255.0 * std), mean / std


def _linear_srl_fail(what, rc):
    raise SrlHipError("{} failed ({}): {}".format(what, rc, load().srlhip_linear_srl_last_error().decode()))


def _tables(scale, offset):
    scale, offset = np.ascontiguousarray(scale, dtype=np.float64).reshape(-1), np.ascontiguousarray(offset, dtype=np.float64).reshape(-1)
    if len(scale) != len(offset):
        raise ValueError("scale and offset must have one entry per channel")
    return scale, offset


def _adam_args(adam):
    return [ctypes.c_double(float(adam[k])) for k in ("lr", "beta1", "beta2", "eps", "bc1", "bc2")]


def adam_at(t, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    """the hyper-parameters of Adam's step t = 1, 2, ... as srlhip_linear_srl_step takes them: bc1 = 1 - beta1^t, bc2 = 1 - beta2^t
    (Python float powers, the way torch.optim.Adam computes them)"""
    return {"lr": lr, "beta1": beta1, "beta2": beta2, "eps": eps, "bc1": 1 - beta1 ** t, "bc2": 1 - beta2 ** t}


def linear_srl_forward(device_id, frames_ptr, n, n_features, state_dim, scale, offset, v_ptr, c_ptr, states_ptr, workspace_ptr, stream=None):
    """srlhip_linear_srl_forward: states float64 [n][S] of the device-resident uint8 frames [n][F].  Raw device pointers; scale / offset
    are host arrays [C]; a workspace of linear_srl_workspace_bytes, 16-byte aligned; enqueue-only on `stream`."""
    scale, offset = _tables(scale, offset)
    rc = load().srlhip_linear_srl_forward(int(device_id), _ptr(frames_ptr), int(n), int(n_features), int(state_dim), len(scale), _ptr(scale),
                                          _ptr(offset), _ptr(v_ptr), _ptr(c_ptr), _ptr(states_ptr), _ptr(workspace_ptr),
                                          ctypes.c_void_p(int(stream)) if stream else None)
    if rc:
        _linear_srl_fail("srlhip_linear_srl_forward", rc)


def linear_srl_step(device_id, frames_ptr, n, n_features, state_dim, scale, offset, g_ptr, v_ptr, m_ptr, v2_ptr, adam, grad_out_ptr=None, stream=None):
    """srlhip_linear_srl_step: ONE launch that forms g = xn^T G and applies Adam to V, m, v [F][S] in place (adam: the dict of adam_at);
    with grad_out_ptr g is also stored.  Raw device pointers; enqueue-only on `stream`."""
    scale, offset = _tables(scale, offset)
    rc = load().srlhip_linear_srl_step(int(device_id), _ptr(frames_ptr), int(n), int(n_features), int(state_dim), len(scale), _ptr(scale),
                                       _ptr(offset), _ptr(g_ptr), _ptr(v_ptr), _ptr(m_ptr), _ptr(v2_ptr), *(_adam_args(adam) + [
                                           _ptr(grad_out_ptr), ctypes.c_void_p(int(stream)) if stream else None]))
    if rc:
        _linear_srl_fail("srlhip_linear_srl_step", rc)


def linear_srl_forward_host(frames, scale, offset, V, c):
    """srlhip_linear_srl_forward_host: the kernel's own arithmetic (csrc/linear_srl.hpp) on the CPU.  frames uint8 [n][...] (flattened to
    [n][F]), V float64 [F][S], c [S] -> float64 [n][S]"""
    scale, offset = _tables(scale, offset)
    V, c = np.ascontiguousarray(V, dtype=np.float64), np.ascontiguousarray(c, dtype=np.float64)
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n = len(frames)
    frames = frames.reshape(n, -1)
    if V.ndim != 2 or frames.shape[1] != V.shape[0] or c.shape != (V.shape[1],):
        raise ValueError("linear_srl_forward_host takes frames [n][F], V [F][S], c [S]")
    out = np.zeros((n, V.shape[1]), np.float64)
    rc = load().srlhip_linear_srl_forward_host(_ptr(frames), n, V.shape[0], V.shape[1], len(scale), _ptr(scale), _ptr(offset), _ptr(V), _ptr(c), _ptr(out))
    if rc:
        _linear_srl_fail("srlhip_linear_srl_forward_host", rc)
    return out


def linear_srl_step_host(frames, scale, offset, G, V, m, v, adam, grad_out=None):
    """srlhip_linear_srl_step_host: gradient + Adam on the CPU, IN PLACE on the float64 C-contiguous arrays V, m, v [F][S]; grad_out
    (float64 [F][S], optional) receives g"""
    scale, offset = _tables(scale, offset)
    frames = np.ascontiguousarray(frames, dtype=np.uint8)
    n = len(frames)
    frames = frames.reshape(n, -1)
    G = np.ascontiguousarray(G, dtype=np.float64)
    for a in (V, m, v) + (() if grad_out is None else (grad_out,)):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.shape == V.shape):
            raise ValueError("linear_srl_step_host updates float64 C-contiguous arrays [F][S] in place")
    if V.ndim != 2 or frames.shape[1] != V.shape[0] or G.shape != (n, V.shape[1]):
        raise ValueError("linear_srl_step_host takes frames [n][F], G [n][S], V [F][S]")
    rc = load().srlhip_linear_srl_step_host(_ptr(frames), n, V.shape[0], V.shape[1], len(scale), _ptr(scale), _ptr(offset), _ptr(G), _ptr(V),
                                            _ptr(m), _ptr(v), *(_adam_args(adam) + [_ptr(grad_out)]))
    if rc:
        _linear_srl_fail("srlhip_linear_srl_step_host", rc)
