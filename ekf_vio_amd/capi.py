"""ctypes binding of libekfvio_hip.so (include/ekfvio.h).  No fallback: a missing or
unloadable library raises; nothing in this package computes on the CPU.

Two builds of the same sources (ekf_vio_amd/_build.py): the product library, which exports exactly what include/ekfvio.h
declares, and libekfvio_hip_hooks.so, which adds include/ekfvio_test_hooks.h (raw kernels, in-kernel stamps, fault
injection: tests and profiling scripts only).  load() is the product; load(hooks=True) the other."""
import ctypes as C
import os

from . import _build

OK, EINVAL, ENUMERIC, ECAPACITY, EDEVICE, ESTATE, EABORTED = range(7)
_ERR = {EINVAL: "EKFVIO_EINVAL", ENUMERIC: "EKFVIO_ENUMERIC", ECAPACITY: "EKFVIO_ECAPACITY",
        EDEVICE: "EKFVIO_EDEVICE", ESTATE: "EKFVIO_ESTATE", EABORTED: "EKFVIO_EABORTED"}
PREDICT_STRUCTURED, PREDICT_DENSE = 0, 1


class Config(C.Structure):
    _fields_ = [("max_features", C.c_int32), ("default_point_depth", C.c_float),
                ("default_point_depth_variance", C.c_float), ("default_point_homogenous_variance", C.c_float),
                ("predict_mode", C.c_int32), ("klt_window_size", C.c_int32), ("klt_max_pyramid_level", C.c_int32),
                ("klt_max_iterations", C.c_int32), ("klt_epsilon", C.c_float), ("klt_min_eigen", C.c_float),
                ("kill_pad", C.c_int32), ("max_image_width", C.c_int32), ("max_image_height", C.c_int32),
                ("use_principal_point", C.c_int32), ("inverse_image_scale", C.c_int32), ("fast_threshold", C.c_int32),
                ("min_new_feature_dist", C.c_int32), ("fast_blur_sigma", C.c_float), ("replenish", C.c_int32),
                ("sample_based_uncertainty", C.c_int32), ("use_imu", C.c_int32), ("imu_gyro_variance", C.c_float),
                ("imu_accel_variance", C.c_float), ("gravity", C.c_float * 3),
                ("klt_fb_max_px", C.c_float), ("remove_lost", C.c_int32)]


class EkfvioError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__("%s %s" % (_ERR.get(code, str(code)), msg))
        self.code = code


# every symbol include/ekfvio.h declares
SYMBOLS = ["ekfvio_default_config", "ekfvio_create", "ekfvio_destroy", "ekfvio_reset", "ekfvio_last_error",
           "ekfvio_add_features", "ekfvio_process", "ekfvio_linearize", "ekfvio_update", "ekfvio_measurement_map",
           "ekfvio_num_features", "ekfvio_dim", "ekfvio_get_base_mu", "ekfvio_get_features", "ekfvio_get_sigma",
           "ekfvio_get_feature_cov", "ekfvio_get_depth_variance", "ekfvio_set_feature_cov", "ekfvio_metric2pixel_map",
           "ekfvio_pixel2metric_map", "ekfvio_get_odometry", "ekfvio_get_points", "ekfvio_check_sigma", "ekfvio_set_state",
           "ekfvio_remove_features", "ekfvio_klt_push_frame", "ekfvio_klt_track", "ekfvio_klt_track_points", "ekfvio_klt_get_level",
           "ekfvio_klt_uncertainty_points", "ekfvio_step_image", "ekfvio_replenish", "ekfvio_fast_detect", "ekfvio_imu", "ekfvio_imu_update",
           "ekfvio_upload_measurements", "ekfvio_run_uploaded", "ekfvio_synchronize", "ekfvio_profile_enable",
           "ekfvio_profile_reset", "ekfvio_profile_count", "ekfvio_profile_name", "ekfvio_profile_get",
           "ekfvio_profile_update_gemms", "ekfvio_get_counters", "ekfvio_set_gate", "ekfvio_get_gate",
           "ekfvio_set_klt_fb", "ekfvio_get_klt_fb", "ekfvio_klt_track_points_fb", "ekfvio_set_distortion", "ekfvio_rectify_map",
           "ekfvio_set_output_covariance", "ekfvio_get_odometry_covariance", "ekfvio_get_points_covariance", "ekfvio_rotation_error_jacobian",
           "ekfvio_set_mask", "ekfvio_get_mask", "ekfvio_get_mask_hits", "ekfvio_mask_blocked", "ekfvio_set_equalize", "ekfvio_equalize",
           "ekfvio_set_klt_photometric", "ekfvio_klt_project_gradients",
           "ekfvio_get_landmark_ids", "ekfvio_set_ended_export", "ekfvio_get_ended",
           "ekfvio_set_zupt", "ekfvio_zupt_update", "ekfvio_get_zupt", "ekfvio_zupt_decide",
           "ekfvio_set_imu_extrinsics", "ekfvio_get_imu_extrinsics", "ekfvio_set_gravity", "ekfvio_get_gravity",
           "ekfvio_gravity_from_accel", "ekfvio_imu_model",
           "ekfvio_set_camera_model", "ekfvio_get_camera_model", "ekfvio_rectify_map_model", "ekfvio_mask_blocked_model",
           "ekfvio_set_replenish_grid", "ekfvio_get_replenish_grid", "ekfvio_replenish_select",
           "ekfvio_aid_update", "ekfvio_aid", "ekfvio_set_frame_aid", "ekfvio_get_aid", "ekfvio_aid_innovation", "ekfvio_aid_rows_body_velocity"]
MASK_RECTIFY_BORDER = 1  # EKFVIO_MASK_RECTIFY_BORDER
CAMERA_PLUMB_BOB, CAMERA_RATIONAL, CAMERA_EQUIDISTANT = 0, 1, 2  # EKFVIO_CAMERA_*
CAMERA_MODELS = {"plumb_bob": CAMERA_PLUMB_BOB, "rational_polynomial": CAMERA_RATIONAL, "rational": CAMERA_RATIONAL,
                 "equidistant": CAMERA_EQUIDISTANT, "fisheye": CAMERA_EQUIDISTANT}  # CameraInfo.distortion_model's names
# every symbol include/ekfvio_test_hooks.h declares (libekfvio_hip_hooks.so only)
HOOK_SYMBOLS = ["ekfvio_test_klt_padded_level", "ekfvio_test_blurred_level0", "ekfvio_test_gemm", "ekfvio_test_gemm_bench", "ekfvio_test_potrf_stamps",
                "ekfvio_test_sweep_stamps", "ekfvio_test_sweep_fault", "ekfvio_test_sweep_delay", "ekfvio_test_cholesky_solve", "ekfvio_test_plan", "ekfvio_test_persist_grid", "ekfvio_test_t2_pair",
                "ekfvio_test_gemm_plan", "ekfvio_test_predict_plan", "ekfvio_test_run_plan", "ekfvio_test_mem", "ekfvio_test_mem_fail",
                "ekfvio_test_fill_update_scratch", "ekfvio_test_zupt_decide", "ekfvio_test_rectify_map", "ekfvio_test_klt_pixels"]

_libs = {}


def lib_path():
    return _build.LIB_PATH


def load(build_if_missing=True, hooks=False):
    """Loads the HIP library (building it with hipcc first if it is absent); hooks=True: the build with the test hooks."""
    if hooks in _libs:
        return _libs[hooks]
    path = _build.HOOKS_LIB_PATH if hooks else _build.LIB_PATH
    if build_if_missing:
        _build.build(hooks=hooks)  # (the hooks build only when asked for) staleness is decided under the build lock; hipcc cross-compiles gfx950 with or without a GPU
    elif not os.path.exists(path):
        raise FileNotFoundError(path + " not built; run python -m ekf_vio_amd._build")
    lib = C.CDLL(path)
    vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
    fp, u8p, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)
    sig = {
        "ekfvio_default_config": [C.POINTER(Config)],
        "ekfvio_create": [C.POINTER(Config), C.c_int, vp, C.POINTER(vp)],
        "ekfvio_destroy": [vp], "ekfvio_reset": [vp],
        "ekfvio_add_features": [vp, fp, i32], "ekfvio_process": [vp, f32], "ekfvio_linearize": [vp, f32, fp],
        "ekfvio_update": [vp, fp, fp, u8p, i32], "ekfvio_measurement_map": [vp, u8p, i32, ip, ip],
        "ekfvio_num_features": [vp], "ekfvio_dim": [vp], "ekfvio_get_base_mu": [vp, fp],
        "ekfvio_get_features": [vp, fp, fp, u8p], "ekfvio_get_sigma": [vp, fp, i32],
        "ekfvio_get_feature_cov": [vp, i32, fp], "ekfvio_get_depth_variance": [vp, i32, fp],
        "ekfvio_set_feature_cov": [vp, i32, fp], "ekfvio_metric2pixel_map": [fp, fp], "ekfvio_pixel2metric_map": [fp, fp],
        "ekfvio_get_odometry": [vp, fp, fp, fp, fp], "ekfvio_get_points": [vp, fp, fp],
        "ekfvio_check_sigma": [vp, fp, fp], "ekfvio_set_state": [vp, i32, fp, fp, fp, u8p, fp, i32],
        "ekfvio_remove_features": [vp, u8p, i32, ip],
        "ekfvio_klt_push_frame": [vp, u8p, i32, i32, i32, fp], "ekfvio_klt_track": [vp, fp, fp, u8p],
        "ekfvio_klt_track_points": [vp, fp, fp, i32, fp, u8p],
        "ekfvio_klt_uncertainty_points": [vp, fp, fp, i32, fp],
        "ekfvio_klt_get_level": [vp, i32, ip, ip, u8p, C.POINTER(C.c_int16)],
        "ekfvio_step_image": [vp, C.c_double, u8p, i32, i32, i32, fp], "ekfvio_imu": [vp, C.c_double, fp, fp], "ekfvio_imu_update": [vp, fp, fp],
        "ekfvio_replenish": [vp, ip, ip], "ekfvio_fast_detect": [vp, i32, i32, i32, ip, ip, ip],
        "ekfvio_upload_measurements": [vp, i32, fp, fp, u8p], "ekfvio_run_uploaded": [vp, i32, i32, f32],
        "ekfvio_synchronize": [vp], "ekfvio_profile_enable": [vp, i32], "ekfvio_profile_reset": [vp],
        "ekfvio_profile_count": [], "ekfvio_profile_name": [i32],
        "ekfvio_profile_get": [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)],
        "ekfvio_profile_update_gemms": [vp, i32, C.POINTER(C.c_double), C.POINTER(C.c_double)],
        "ekfvio_get_counters": [vp, C.POINTER(C.c_int64)],
        "ekfvio_set_gate": [vp, f32], "ekfvio_get_gate": [vp, fp, u8p, ip, ip, C.POINTER(C.c_int64)],
        "ekfvio_set_klt_fb": [vp, f32], "ekfvio_get_klt_fb": [vp, fp, u8p, ip, ip, C.POINTER(C.c_int64)],
        "ekfvio_klt_track_points_fb": [vp, fp, fp, i32, fp, u8p, fp, fp, u8p],
        "ekfvio_set_distortion": [vp, C.POINTER(C.c_double), i32],
        "ekfvio_rectify_map": [fp, C.POINTER(C.c_double), i32, i32, i32, ip, ip],  # no handle, no device
        "ekfvio_set_output_covariance": [vp, i32], "ekfvio_get_odometry_covariance": [vp, fp, fp], "ekfvio_get_points_covariance": [vp, fp],
        "ekfvio_rotation_error_jacobian": [fp, fp],  # no handle, no device
        "ekfvio_set_mask": [vp, u8p, i32, i32, i32, i32], "ekfvio_get_mask": [vp, u8p, i32, ip, ip], "ekfvio_get_mask_hits": [vp, u8p, ip, ip],
        "ekfvio_mask_blocked": [fp, C.POINTER(C.c_double), i32, u8p, i32, i32, i32, i32, i32, i32, u8p],  # no handle, no device
        "ekfvio_set_equalize": [vp, f32, i32, i32],
        "ekfvio_equalize": [u8p, i32, i32, i32, f32, i32, i32, u8p],  # no handle, no device
        "ekfvio_set_klt_photometric": [vp, i32],
        "ekfvio_klt_project_gradients": [ip, ip, ip, i32, ip, ip],  # no handle, no device
        "ekfvio_get_landmark_ids": [vp, C.POINTER(C.c_int64), C.POINTER(C.c_double)],
        "ekfvio_set_ended_export": [vp, i32],
        "ekfvio_get_ended": [vp, C.POINTER(C.c_int64), C.POINTER(C.c_double), ip, fp, fp, i32, ip, C.POINTER(C.c_int64)],
        "ekfvio_set_zupt": [vp, f32, i32, f32, f32, f32], "ekfvio_zupt_update": [vp, f32, f32],
        "ekfvio_get_zupt": [vp, fp, ip, ip, ip, ip, C.POINTER(C.c_int64)],
        "ekfvio_zupt_decide": [fp, fp, u8p, i32, f32, i32, f32, fp, ip, ip, ip],  # no handle, no device
        "ekfvio_set_imu_extrinsics": [vp, fp, fp], "ekfvio_get_imu_extrinsics": [vp, fp, fp, ip],
        "ekfvio_set_gravity": [vp, fp], "ekfvio_get_gravity": [vp, fp],
        "ekfvio_gravity_from_accel": [fp, C.POINTER(C.c_double), f32, fp],  # no handle, no device
        "ekfvio_imu_model": [fp, fp, fp, fp, fp, fp, fp, fp],  # no handle, no device
        "ekfvio_set_camera_model": [vp, i32, C.POINTER(C.c_double), i32, fp],
        "ekfvio_get_camera_model": [vp, ip, C.POINTER(C.c_double), ip, fp, ip, ip],
        "ekfvio_rectify_map_model": [fp, i32, C.POINTER(C.c_double), i32, fp, i32, i32, ip, ip],  # no handle, no device
        "ekfvio_mask_blocked_model": [fp, i32, C.POINTER(C.c_double), i32, fp, u8p, i32, i32, i32, i32, i32, i32, u8p],  # no handle, no device
        "ekfvio_set_replenish_grid": [vp, i32, i32], "ekfvio_get_replenish_grid": [vp, ip, ip],
        "ekfvio_replenish_select": [ip, ip, i32, ip, i32, u8p, i32, i32, i32, i32, i32, i32, i32, ip, ip],  # no handle, no device
        "ekfvio_aid_update": [vp, i32, fp, fp, fp, f32], "ekfvio_aid": [vp, C.c_double, i32, fp, fp, fp, f32],
        "ekfvio_set_frame_aid": [vp, i32, fp, fp, fp, f32], "ekfvio_get_aid": [vp, fp, ip, C.POINTER(C.c_int64), C.POINTER(C.c_int64)],
        "ekfvio_aid_innovation": [fp, fp, i32, fp, fp, fp, fp, fp, fp, ip],  # no handle, no device
        "ekfvio_aid_rows_body_velocity": [fp, fp, fp, fp, fp, fp, fp],  # no handle, no device
    }
    if hooks:
        sig.update({
            "ekfvio_test_klt_padded_level": [vp, i32, ip, u8p, C.POINTER(C.c_int16)],
            "ekfvio_test_blurred_level0": [vp, u8p],
            "ekfvio_test_gemm": [vp, i32, i32, i32, i32, f32, fp, i32, fp, i32, f32, fp, i32, i32],
            "ekfvio_test_cholesky_solve": [vp, i32, i32, fp, fp, fp, fp, ip],
            "ekfvio_test_potrf_stamps": [vp, C.POINTER(C.c_int64)],
            "ekfvio_test_sweep_stamps": [vp, C.c_int, C.POINTER(C.c_int64)],
            "ekfvio_test_sweep_fault": [vp, i32, i32],
            "ekfvio_test_sweep_delay": [vp, i32, i32, i32],
            "ekfvio_test_gemm_bench": [vp, i32, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_double)],
            "ekfvio_test_plan": [i32] * 8 + [f32, ip],  # no handle: csrc/plan.h's plan_update, on any machine
            "ekfvio_test_persist_grid": [i32] * 8 + [f32, ip, i32, ip],  # ... and the PersistGrid / PersistFlags of that plan
            "ekfvio_test_t2_pair": [i32, ip],
            "ekfvio_test_gemm_plan": [i32] * 11 + [ip],  # ... plan_gemm and plan_predict
            "ekfvio_test_predict_plan": [i32] * 5 + [ip],
            "ekfvio_test_run_plan": [i32] * 4 + [ip, i32, ip],  # ... and plan_run
            "ekfvio_test_mem": [vp, C.POINTER(C.c_int64)],  # csrc/mem.h: what a handle's ledger holds (None: the whole library copy)
            "ekfvio_test_mem_fail": [vp, i32],
            "ekfvio_test_fill_update_scratch": [vp, C.c_uint32],  # a word into the update's float work buffers: a handle with a history
            "ekfvio_test_zupt_decide": [vp, fp, fp, u8p, i32, f32, i32, f32, fp, ip, ip, ip],  # the device's zero-velocity decision on arbitrary points
            "ekfvio_test_rectify_map": [vp, ip, ip, i32, ip, ip],  # the rectification map as the device holds it
            "ekfvio_test_klt_pixels": [vp, fp, fp, i32],  # the tracker's pixel buffers behind the landmarks' last track
        })
    for name, args in sig.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.ekfvio_last_error.argtypes = [vp]
    lib.ekfvio_last_error.restype = C.c_char_p
    lib.ekfvio_profile_name.restype = C.c_char_p
    _libs[hooks] = lib
    return lib
