"""ctypes binding of include/mpc_amd.h (the drop-in C ABI)."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

MAX_TABLE = 16
NW = 12
NCOEF = 5
NSTATE = 6
NOUT = 9
MAX_N = 64
ABI_VERSION = 5
PRECISION_F64, PRECISION_F32 = 0, 1

STATUS_NAMES = {0: "success", 1: "maxiter", 2: "linesearch", 3: "infeasible", 4: "numeric", 5: "pending", 6: "acceptable"}
ERR_NAMES = {0: "MPC_OK", -1: "MPC_ERR_INVALID", -2: "MPC_ERR_NO_DEVICE", -3: "MPC_ERR_HIP",
             -4: "MPC_ERR_UNSUPPORTED", -5: "MPC_ERR_IO"}


class MpcError(RuntimeError):
    pass


class MpcParams(C.Structure):
    """Mirror of ``struct MpcParams`` (include/mpc_amd.h); field order is ABI."""
    _fields_ = [
        ("abi_version", C.c_int32), ("N", C.c_int32), ("dt", C.c_double), ("Lf", C.c_double),
        ("weights", C.c_double * NW), ("cte_panic", C.c_double), ("epsi_panic", C.c_double),
        ("max_steering", C.c_double), ("max_acceleration", C.c_double), ("max_deceleration", C.c_double),
        ("max_speed", C.c_double), ("n_steers", C.c_int32), ("n_steer_speeds", C.c_int32),
        ("steers", C.c_double * MAX_TABLE), ("steer_speeds", C.c_double * MAX_TABLE),
        ("n_yaw_changes", C.c_int32), ("n_yaw_change_speeds", C.c_int32),
        ("yaw_changes", C.c_double * MAX_TABLE), ("yaw_change_speeds", C.c_double * MAX_TABLE),
        ("max_fit_order", C.c_int32), ("latency_ms", C.c_int32), ("max_fit_error", C.c_double),
        ("lookahead", C.c_double), ("steer_adj_thresh", C.c_double), ("steer_adj_ratio", C.c_double),
        ("ipopt_timeout", C.c_double), ("branch_mode", C.c_int32), ("precision", C.c_int32),
        ("max_iter", C.c_int32), ("pass_cut", C.c_int32), ("tol", C.c_double),
        ("out_step_tol", C.c_double), ("tol_f32", C.c_double), ("polish", C.c_int32),
        ("pass_cut_next", C.c_int32 * 3), ("honor_original_bounds", C.c_int32), ("bound_relax_factor", C.c_double),
        ("tail_cut", C.c_int32), ("tail_ring", C.c_int32), ("tail_capacity", C.c_int64),
        ("f32_finish", C.c_int32), ("f64_f32_start", C.c_int32), ("mixed_switch_mu", C.c_double),
        ("lane_compact", C.c_int32), ("f32_phase_refill", C.c_int32), ("acceptable_iter", C.c_int32),
        ("dual_inf_tol", C.c_double), ("constr_viol_tol", C.c_double), ("compl_inf_tol", C.c_double),
        ("acceptable_tol", C.c_double), ("acceptable_dual_inf_tol", C.c_double),
        ("acceptable_constr_viol_tol", C.c_double), ("acceptable_compl_inf_tol", C.c_double), ("initial_state_rows", C.c_int32), ("wave_max_batch", C.c_int32),
        ("max_soc", C.c_int32),
    ]

    def copy(self):
        q = MpcParams()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(MpcParams))
        return q


class MpcWireTelemetry(C.Structure):
    _fields_ = [("x", C.c_double), ("y", C.c_double), ("psi", C.c_double), ("speed", C.c_double),
                ("steering_angle", C.c_double), ("throttle", C.c_double), ("npts", C.c_int32), ("reserved", C.c_int32),
                ("ptsx", C.c_double * 8), ("ptsy", C.c_double * 8)]


class MpcBatchStats(C.Structure):
    _fields_ = [("batch", C.c_int64), ("n_success", C.c_int64), ("n_maxiter", C.c_int64),
                ("n_linesearch", C.c_int64), ("n_infeasible", C.c_int64), ("n_numeric", C.c_int64), ("n_acceptable", C.c_int64),
                ("iter_sum", C.c_int64), ("iter_max", C.c_int32), ("n_pending", C.c_int32),
                ("kernel_ms", C.c_double)]


NMODEL = 6       # MPC_NMODEL: rows of a model array, [NMODEL][ld] (the mpc_*_model entry points), in the order of MODEL_ROWS
MODEL_DT, MODEL_LF, MODEL_MAX_STEERING, MODEL_MAX_ACCELERATION, MODEL_MAX_DECELERATION, MODEL_MAX_SPEED = range(6)
MODEL_ROWS = ("dt", "Lf", "max_steering", "max_acceleration", "max_deceleration", "max_speed")   # the MpcParams fields, row by row

WARM_REC = 22    # MPC_WARM_REC: reals per stage of a warm buffer (s 6, u 2, lam 6, z_L 4, z_U 4)


class MpcWarmOpts(C.Structure):
    """Mirror of ``struct MpcWarmOpts`` (include/mpc_amd.h)."""
    _fields_ = [("size", C.c_int32), ("shift", C.c_int32), ("mu_init", C.c_double), ("bound_push", C.c_double),
                ("duals", C.c_int32), ("reserved", C.c_int32)]


# every symbol include/mpc_amd.h declares (checked by tests/test_abi.py)
EXPORTS = ["mpc_params_default", "mpc_params_load_json", "mpc_create", "mpc_set_params", "mpc_destroy",
           "mpc_last_error", "mpc_abi_version", "mpc_solve_batch_device", "mpc_solve_batch_host",
           "mpc_synchronize", "mpc_get_stats", "mpc_debug_math", "mpc_run_batch_device",
           "mpc_telemetry_batch_device", "mpc_rollout_batch_device", "mpc_debug_math_ext", "mpc_debug_math_all",
           "mpc_solve_batch_device_f32", "mpc_wire_parse", "mpc_wire_format_steer", "mpc_wire_format_manual",
           "mpc_wire_telemetry_batch_host", "mpc_telemetry_batch_host", "mpc_handle_device",
           "mpc_run_batch_host", "mpc_last_batch_id", "mpc_tail_poll", "mpc_tail_wait", "mpc_tail_stream_wait", "mpc_tail_flush", "mpc_tail_pending", "mpc_tail_info", "mpc_solve_batch_host_f32", "mpc_inflight_advice", "mpc_take_order_info",
           "mpc_warm_rows", "mpc_warm_opts_default", "mpc_solve_batch_device_warm", "mpc_solve_batch_host_warm",
           "mpc_rollout_batch_device_warm", "mpc_run_batch_device_warm", "mpc_run_batch_host_warm",
           "mpc_telemetry_batch_device_warm", "mpc_telemetry_batch_host_warm", "mpc_wire_telemetry_batch_host_warm",
           "mpc_rollout_batch_device_fused", "mpc_rollout_fused_info",
           "mpc_solve_batch_device_model", "mpc_solve_batch_host_model", "mpc_rollout_batch_device_model",
           "mpc_solve_batch_device_warm_model", "mpc_solve_batch_host_warm_model", "mpc_rollout_batch_device_warm_model",
           "mpc_rollout_batch_device_fused_model",
           "mpc_run_batch_device_model", "mpc_run_batch_host_model", "mpc_telemetry_batch_device_model", "mpc_telemetry_batch_host_model",
           "mpc_run_batch_device_warm_model", "mpc_run_batch_host_warm_model", "mpc_telemetry_batch_device_warm_model",
           "mpc_telemetry_batch_host_warm_model", "mpc_wire_telemetry_batch_host_model", "mpc_wire_telemetry_batch_host_warm_model"]
# ... and every symbol include/mpc_amd_horizon.h declares (the part of the header that mpc_amd.h includes; tests/test_horizon.py)
HORIZON_EXPORTS = ["mpc_solve_batch_device_horizon", "mpc_solve_batch_host_horizon", "mpc_solve_batch_device_warm_horizon",
                   "mpc_solve_batch_host_warm_horizon", "mpc_rollout_batch_device_horizon", "mpc_rollout_batch_device_warm_horizon",
                   "mpc_rollout_batch_device_fused_horizon"]
# ... and include/mpc_amd_certify.h (the certificate of a stored point; tests/test_certify.py)
CERTIFY_EXPORTS = ["mpc_certify_batch_device", "mpc_certify_batch_host"]
NCERT = 12       # MPC_NCERT: rows of cert [NCERT][ld], in the order of CERT_ROWS
(CERT_OBJ, CERT_CONSTR_VIOL, CERT_DUAL_INF, CERT_COMPL, CERT_NLP_ERROR, CERT_BOUND_VIOL, CERT_OBJ_SCALING, CERT_COST_CTE, CERT_COST_EPSI,
 CERT_COST_V, CERT_COST_DELTA, CERT_COST_DDELTA) = range(NCERT)
CERT_ROWS = ("obj", "constr_viol", "dual_inf", "compl", "nlp_error", "bound_viol", "obj_scaling", "cost_cte", "cost_epsi", "cost_v",
             "cost_delta", "cost_ddelta")
CERT_CONVERGED, CERT_ACCEPTABLE, CERT_NOT_CONVERGED, CERT_NOT_A_POINT, CERT_NO_PROBLEM = range(5)
CERT_VERDICT_NAMES = {0: "converged", 1: "acceptable", 2: "not_converged", 3: "not_a_point", 4: "no_problem"}

# ... and include/mpc_amd_drive.h (track driving; tests/test_drive.py)
DRIVE_EXPORTS = ["mpc_drive_opts_default", "mpc_drive_batch_device", "mpc_drive_batch_device_fused", "mpc_drive_batch_host", "mpc_drive_info",
                 "mpc_drive_batch_device_model", "mpc_drive_batch_device_fused_model", "mpc_drive_batch_host_model",
                 "mpc_drive_batch_device_latency", "mpc_drive_batch_device_fused_latency", "mpc_drive_batch_host_latency",
                 "mpc_telemetry_batch_device_latency", "mpc_telemetry_batch_host_latency",
                 "mpc_drive_batch_device_horizon", "mpc_drive_batch_device_fused_horizon", "mpc_drive_batch_host_horizon",
                 "mpc_telemetry_batch_device_horizon", "mpc_telemetry_batch_host_horizon",
                 "mpc_drive_plant_default", "mpc_drive_batch_device_plant", "mpc_drive_batch_device_fused_plant", "mpc_drive_batch_host_plant"]
NPLANT = 6       # MPC_NPLANT: rows of a plant array, [NPLANT][ld] (the mpc_drive_*_plant entry points)
PLANT_LF, PLANT_STEER_GAIN, PLANT_STEER_BIAS, PLANT_ACCEL_GAIN, PLANT_DRAG_SPEED, PLANT_DRIFT = range(NPLANT)
# ... and include/mpc_amd_noise.h (the track drive under noise; tests/test_drive_noise.py)
NOISE_EXPORTS = ["mpc_drive_batch_device_noise", "mpc_drive_batch_device_fused_noise", "mpc_drive_batch_host_noise", "mpc_drive_noise_default",
                 "mpc_drive_noise_draw", "mpc_debug_philox4x32", "mpc_debug_drive_noise_device"]
NNOISE = 7       # MPC_NNOISE: rows of a noise array, [NNOISE][ld] (the mpc_drive_*_noise entry points)
NOISE_SEED, NOISE_POS, NOISE_PSI, NOISE_SPEED, NOISE_STEER, NOISE_DRIFT, NOISE_DROP = range(NNOISE)
DRAW_Z_X, DRAW_Z_Y, DRAW_Z_PSI, DRAW_Z_SPEED, DRAW_Z_STEER, DRAW_Z_DRIFT, DRAW_U_DROP = range(7)      # MPC_DRAW_*: rows of a draw
NLATENCY = 3     # MPC_NLATENCY: rows of a latency array, [NLATENCY][ld] (the mpc_drive_*_latency entry points)
LATENCY_COMP, LATENCY_SUB_OLD, LATENCY_SUB_NEW = range(NLATENCY)
DRIVE_MAX_TRACK, DRIVE_NSUM, DRIVE_REC = 4096, 8, 13      # MPC_DRIVE_MAX_TRACK, rows of summary [NSUM][ld], rows of a step of hist [REC][ld]
(DRIVE_SUM_MAX_CTE, DRIVE_SUM_CTE2, DRIVE_SUM_MAX_EPSI, DRIVE_SUM_SPEED, DRIVE_SUM_MIN_SPEED, DRIVE_SUM_PROGRESS, DRIVE_SUM_FIRST_OFF,
 DRIVE_SUM_FAILED) = range(DRIVE_NSUM)
DRIVE_REC_CAR, DRIVE_REC_CMD, DRIVE_REC_CTE, DRIVE_REC_EPSI, DRIVE_REC_STATUS, DRIVE_REC_ITERS, DRIVE_REC_K = 0, 6, 8, 9, 10, 11, 12


class MpcDriveOpts(C.Structure):
    """Mirror of ``struct MpcDriveOpts`` (include/mpc_amd_drive.h)."""
    _fields_ = [("size", C.c_int32), ("npts", C.c_int32), ("sub_old", C.c_int32), ("sub_new", C.c_int32), ("warm_start", C.c_int32),
                ("reserved", C.c_int32), ("h", C.c_double), ("extra_latency", C.c_double), ("cte_limit", C.c_double)]


_lib = None


def library_path():
    return os.path.join(HERE, "lib", "libmpc_amd.so")


def build_library(verbose=False):
    """Compile the HIP extension for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)
    return library_path()


def library():
    """Load the product library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise MpcError("HIP extension %s is missing: run __graft_entry__.build() (there is no CPU fallback)" % path)
    # One HIP runtime per process: torch wheels bundle their own libamdhip64 (same soname as /opt/rocm's).  If this
    # library were loaded first it would bind /opt/rocm's copy, and torch, imported later, would then fail to see a
    # device.  Importing torch first makes both use the copy torch ships.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    DP = C.c_void_p
    L.mpc_params_default.argtypes = [C.POINTER(MpcParams)]
    L.mpc_params_load_json.argtypes = [C.c_char_p, C.POINTER(MpcParams)]
    L.mpc_create.argtypes = [C.POINTER(MpcParams), C.c_int, C.c_int64, C.POINTER(C.c_void_p)]
    L.mpc_set_params.argtypes = [C.c_void_p, C.POINTER(MpcParams)]
    L.mpc_destroy.argtypes = [C.c_void_p]
    L.mpc_destroy.restype = None
    L.mpc_last_error.restype = C.c_char_p
    L.mpc_abi_version.restype = C.c_int
    L.mpc_synchronize.argtypes = [C.c_void_p]
    L.mpc_get_stats.argtypes = [C.c_void_p, C.POINTER(MpcBatchStats)]
    L.mpc_debug_math.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 4
    L.mpc_debug_math_ext.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 6
    L.mpc_debug_math_all.argtypes = [C.c_int, C.c_int64] + [C.c_void_p] * 3
    L.mpc_handle_device.argtypes = [C.c_void_p]
    L.mpc_inflight_advice.argtypes = [C.c_void_p, C.c_int64]
    L.mpc_inflight_advice.restype = C.c_int
    L.mpc_last_batch_id.argtypes = [C.c_void_p]
    L.mpc_last_batch_id.restype = C.c_int64
    L.mpc_tail_wait.argtypes = [C.c_void_p, C.c_int64]
    L.mpc_tail_poll.argtypes = [C.c_void_p, C.c_int64]
    L.mpc_tail_stream_wait.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.mpc_tail_flush.argtypes = [C.c_void_p]
    L.mpc_tail_pending.argtypes = [C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    L.mpc_tail_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.mpc_take_order_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.mpc_warm_rows.argtypes = [C.c_int]
    L.mpc_warm_rows.restype = C.c_int64
    L.mpc_warm_opts_default.argtypes = [C.POINTER(MpcWarmOpts)]
    L.mpc_rollout_fused_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    # The batch entry points: one row per family -- (head, outs, stream or not) -- and the rule of include/mpc_amd.h for its four forms:
    # _model puts `model` (one pointer) behind the head, _warm puts `warm` (warm_in, warm_status, warm_out, ld_warm, opts; the
    # stepwise rollout: opts alone) behind that.  The fused rollout has two forms: its warm_start, opts pair leads its outs.
    # A third rule for the families marked so (the solve and the rollouts): _horizon is _model plus `horizon` (one pointer) behind `model`.
    I64, OPTS = C.c_int64, C.POINTER(MpcWarmOpts)
    H = [C.c_void_p, I64, I64]
    WARM = [DP] * 3 + [I64, OPTS]
    families = [("mpc_solve_batch_device", H + [DP] * 5, [DP] * 4, True, WARM, True),
                ("mpc_solve_batch_host", H + [DP] * 5, [DP] * 4, False, WARM, True),
                ("mpc_run_batch_device", H + [C.c_int] + [DP] * 3, [DP] * 5, True, WARM, False),
                ("mpc_run_batch_host", H + [C.c_int] + [DP] * 3, [DP] * 5, False, WARM, False),
                ("mpc_telemetry_batch_device", H + [C.c_int, DP, C.c_double] + [DP] * 2, [DP] * 3, True, WARM, False),
                ("mpc_telemetry_batch_host", H + [C.c_int, DP, C.c_double] + [DP] * 2, [DP] * 2, False, WARM, False),
                ("mpc_wire_telemetry_batch_host", [C.c_void_p, I64, C.POINTER(MpcWireTelemetry), DP, C.c_double], [DP] * 2, False, WARM, False),
                ("mpc_rollout_batch_device", H + [C.c_int] + [DP] * 5, [DP] * 3, True, [OPTS], True),
                ("mpc_rollout_batch_device_fused", H + [C.c_int] + [DP] * 5, [C.c_int, OPTS] + [DP] * 3, True, None, True)]
    for family, head, outs, stream, warm, has_horizon in families:
        tail = outs + ([C.c_void_p] if stream else [])
        for w_name, w in [("", [])] + ([("_warm", warm)] if warm else []):
            for m_name, m in (("", []), ("_model", [DP])) + ((("_horizon", [DP, DP]),) if has_horizon else ()):
                getattr(L, family + w_name + m_name).argtypes = head + m + w + tail
    # the certificate: the _horizon solve's inputs, then sol, ld_sol, cert, verdict (and the stream)
    L.mpc_certify_batch_host.argtypes = H + [DP] * 7 + [DP, I64, DP, DP]
    L.mpc_certify_batch_device.argtypes = L.mpc_certify_batch_host.argtypes + [C.c_void_p]
    # track driving: B, ld, steps, car, track_x, track_y, n_track, weights, opts, warm_opts, summary, hist, status, iters (and the stream)
    L.mpc_drive_opts_default.argtypes = [C.POINTER(MpcParams), C.POINTER(MpcDriveOpts)]
    L.mpc_drive_batch_host.argtypes = H + [C.c_int] + [DP] * 3 + [C.c_int, DP, C.POINTER(MpcDriveOpts), OPTS] + [DP] * 4
    L.mpc_drive_batch_device.argtypes = L.mpc_drive_batch_host.argtypes + [C.c_void_p]
    L.mpc_drive_batch_device_fused.argtypes = L.mpc_drive_batch_device.argtypes
    # ... and their _model forms: `model` (one pointer) directly behind `weights`
    drive_head = H + [C.c_int] + [DP] * 3 + [C.c_int, DP]
    for name in ("mpc_drive_batch_host", "mpc_drive_batch_device", "mpc_drive_batch_device_fused"):
        getattr(L, name + "_model").argtypes = drive_head + [DP] + getattr(L, name).argtypes[len(drive_head):]
    # ... and their _latency forms: `latency` (one pointer) directly behind `model`; the telemetry handler's: the _warm_model form plus
    # `comp` (one pointer) directly behind extra_latency
    for name in ("mpc_drive_batch_host", "mpc_drive_batch_device", "mpc_drive_batch_device_fused"):
        getattr(L, name + "_latency").argtypes = drive_head + [DP, DP] + getattr(L, name).argtypes[len(drive_head):]
    tel_head = H + [C.c_int, DP, C.c_double]
    for name in ("mpc_telemetry_batch_device", "mpc_telemetry_batch_host"):
        getattr(L, name + "_latency").argtypes = tel_head + [DP] + getattr(L, name + "_warm_model").argtypes[len(tel_head):]
    # ... and the _horizon forms of both: the _latency form plus `horizon` (one pointer) directly behind `model`
    for name in ("mpc_drive_batch_host", "mpc_drive_batch_device", "mpc_drive_batch_device_fused"):
        at = len(drive_head) + 1
        getattr(L, name + "_horizon").argtypes = getattr(L, name + "_latency").argtypes[:at] + [DP] + getattr(L, name + "_latency").argtypes[at:]
    for name in ("mpc_telemetry_batch_device", "mpc_telemetry_batch_host"):
        at = len(tel_head) + 4      # (comp, ptsx, ptsy, model)
        getattr(L, name + "_horizon").argtypes = getattr(L, name + "_latency").argtypes[:at] + [DP] + getattr(L, name + "_latency").argtypes[at:]
    # ... and the drive's _plant forms: the _horizon form plus `plant` (one pointer) directly behind `latency`
    for name in ("mpc_drive_batch_host", "mpc_drive_batch_device", "mpc_drive_batch_device_fused"):
        at = len(drive_head) + 3      # (model, horizon, latency)
        getattr(L, name + "_plant").argtypes = getattr(L, name + "_horizon").argtypes[:at] + [DP] + getattr(L, name + "_horizon").argtypes[at:]
    # ... and the _budget forms (include/mpc_amd_budget.h): `budget` (one pointer) directly behind `horizon` -- of the drive's _plant forms
    # and of the solve's _warm_horizon forms
    for name in ("mpc_drive_batch_host", "mpc_drive_batch_device", "mpc_drive_batch_device_fused"):
        at = len(drive_head) + 2      # (model, horizon)
        getattr(L, name + "_budget").argtypes = getattr(L, name + "_plant").argtypes[:at] + [DP] + getattr(L, name + "_plant").argtypes[at:]
    for name in ("mpc_solve_batch_device", "mpc_solve_batch_host"):
        at = len(H) + 5 + 2           # (state .. weights, model, horizon)
        getattr(L, name + "_budget").argtypes = getattr(L, name + "_warm_horizon").argtypes[:at] + [DP] + getattr(L, name + "_warm_horizon").argtypes[at:]
    # ... and the drive's _noise forms (include/mpc_amd_noise.h): the _budget form plus `noise` (one pointer) directly behind `plant` and
    # `seen` (one pointer) directly behind `hist`
    for name in ("mpc_drive_batch_host", "mpc_drive_batch_device", "mpc_drive_batch_device_fused"):
        a = getattr(L, name + "_budget").argtypes
        at = len(drive_head) + 5      # (model, horizon, budget, latency, plant)
        getattr(L, name + "_noise").argtypes = a[:at] + [DP] + a[at:at + 4] + [DP] + a[at + 4:]      # (opts, warm_opts, summary, hist | seen)
    L.mpc_drive_noise_default.argtypes = [DP]
    L.mpc_drive_noise_draw.argtypes = [C.c_double, C.c_int32, DP]
    L.mpc_debug_philox4x32.argtypes = [DP, DP, DP]
    L.mpc_debug_drive_noise_device.argtypes = [C.c_void_p, I64, DP, DP, DP, C.c_void_p]
    L.mpc_drive_plant_default.argtypes = [C.POINTER(MpcParams), DP]
    L.mpc_drive_info.argtypes = [C.c_void_p, C.POINTER(C.c_int64)]
    L.mpc_solve_batch_device_f32.argtypes = L.mpc_solve_batch_device.argtypes      # (the same pointers, to floats)
    L.mpc_solve_batch_host_f32.argtypes = L.mpc_solve_batch_host.argtypes
    L.mpc_wire_parse.argtypes = [C.c_char_p, C.c_int64, C.POINTER(MpcWireTelemetry)]
    L.mpc_wire_format_steer.argtypes = [C.c_double, C.c_double, C.c_char_p, C.c_int64]
    L.mpc_wire_format_steer.restype = C.c_int64
    L.mpc_wire_format_manual.argtypes = [C.c_char_p, C.c_int64]
    L.mpc_wire_format_manual.restype = C.c_int64
    if L.mpc_abi_version() != ABI_VERSION:
        raise MpcError("ABI version mismatch between %s and the Python binding" % path)
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        msg = library().mpc_last_error()
        raise MpcError("%s failed: %s (%s)" % (what, ERR_NAMES.get(rc, rc), msg.decode() if msg else ""))


def params_default():
    p = MpcParams()
    check(library().mpc_params_default(C.byref(p)), "mpc_params_default")
    return p


def warm_rows(N):
    """mpc_warm_rows: rows of a warm buffer for horizon N, (N-1) * WARM_REC."""
    r = int(library().mpc_warm_rows(int(N)))
    if r < 0:
        raise MpcError("mpc_warm_rows(%d): N out of range" % N)
    return r


def warm_opts_default(**overrides):
    """mpc_warm_opts_default, with keyword overrides (shift=0, mu_init=1e-6 ...)."""
    o = MpcWarmOpts()
    check(library().mpc_warm_opts_default(C.byref(o)), "mpc_warm_opts_default")
    for k, v in overrides.items():
        setattr(o, k, v)
    return o


def warm_to_vars(warm, state, N):
    """One instance's warm column ((N-1) * WARM_REC values) and its state [6] as the reference's decision vector of 8N-2
    entries in the order of MPC.cpp:56-63: x, y, psi, v, cte, epsi (N each; index 0 is the given state), delta, a (N-1 each)."""
    import numpy as np
    rec = np.asarray(warm, dtype=np.float64).reshape(N - 1, WARM_REC)
    v = np.empty(8 * N - 2)
    for q in range(6):
        v[q * N] = state[q]
        v[q * N + 1:(q + 1) * N] = rec[:, q]
    v[6 * N:7 * N - 1] = rec[:, 6]
    v[7 * N - 1:] = rec[:, 7]
    return v


def drive_opts_default(params, **overrides):
    """mpc_drive_opts_default for these parameters (needs no device), with keyword overrides (warm_start=1, sub_new=10 ...)."""
    o = MpcDriveOpts()
    check(library().mpc_drive_opts_default(C.byref(params), C.byref(o)), "mpc_drive_opts_default")
    for k, v in overrides.items():
        setattr(o, k, v)
    return o


def drive_plant_default(params, B=None, model=None):
    """mpc_drive_plant_default for these parameters (needs no device): the column {Lf, 1, 0, 6, 50, 0} under which the plant of the
    mpc_drive_*_plant entry points is the plant of the forms without `plant`.  B = None: the column [NPLANT]; else an array [NPLANT, B]
    of it, row PLANT_LF from ``model`` [6, B] (its Lf row) if one is given."""
    import numpy as np
    col = np.zeros(NPLANT)
    check(library().mpc_drive_plant_default(C.byref(params), col.ctypes.data), "mpc_drive_plant_default")
    if B is None:
        return col
    a = np.ascontiguousarray(np.repeat(col[:, None], int(B), axis=1))
    if model is not None:
        a[PLANT_LF] = np.asarray(model, dtype=np.float64)[MODEL_LF]
    return a


def drive_noise_default(B=None, seeds=None):
    """mpc_drive_noise_default (needs no device): the zero column -- seed 0, every sigma 0, p_drop 0 -- under which a drive with
    ``noise=`` is the drive without.  B = None: the column [NNOISE]; else an array [NNOISE, B] of it, row NOISE_SEED from ``seeds`` [B]
    (integers in [0, 2**53)) if given: the array a caller then sets the sigma rows of."""
    import numpy as np
    col = np.ones(NNOISE)
    check(library().mpc_drive_noise_default(col.ctypes.data), "mpc_drive_noise_default")
    if B is None and seeds is None:
        return col
    if B is None:
        B = len(seeds)
    a = np.ascontiguousarray(np.repeat(col[:, None], int(B), axis=1))
    if seeds is not None:
        sd = np.asarray(seeds)
        if sd.shape != (int(B),) or (sd < 0).any() or (sd >= 2 ** 53).any() or (sd != np.floor(sd)).any():
            raise ValueError("seeds must be B integers in [0, 2**53)")
        a[NOISE_SEED] = sd.astype(np.float64)
    return a


def drive_noise_draw(seed, step):
    """mpc_drive_noise_draw (needs no device): the seven values car `seed` draws at message `step` -- z_x, z_y, z_psi, z_speed,
    z_steer, z_drift, u_drop (rows DRAW_*)."""
    import numpy as np
    out = np.empty(7)
    check(library().mpc_drive_noise_draw(float(seed), int(step), out.ctypes.data), "mpc_drive_noise_draw")
    return out


def inflight_advice(params, B):
    """mpc_inflight_advice: batches of B instances to keep in flight for these parameters."""
    return int(library().mpc_inflight_advice(C.byref(params), int(B)))


def params_from_json(path, **overrides):
    """Config::load(path) (src/utils/Config.cpp:31-87) through the C ABI; keyword overrides
    (e.g. N=25, dt=0.05) are applied afterwards like mpc_main.cpp's CLI overrides."""
    p = MpcParams()
    check(library().mpc_params_load_json(os.fspath(path).encode(), C.byref(p)), "mpc_params_load_json(%s)" % path)
    for k, v in overrides.items():
        if k == "weights":
            for i, w in enumerate(v):
                p.weights[i] = w
        else:
            setattr(p, k, v)
    return p
