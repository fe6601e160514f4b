"""ctypes mirror of include/dab.h (the C ABI of libdab.so).

Only plain structs and the shared-library loader live here. The library is built
in-tree (deeparc-sfm_amd/libdab.so, ``make -C deeparc-sfm_amd``); there is no CPU
fallback — loading fails loudly if the HIP build is missing.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdab.so")

DAB_OK = 0
DAB_LINEAR_SOLVER_EXPLICIT_SCHUR = 0
DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG = 1
DAB_LINEAR_SOLVER_AUTO = 2
DAB_CONVERGENCE = 0
DAB_NO_CONVERGENCE = 1
DAB_FAILURE = 2
TERMINATION = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE"}
DAB_E_INVALID = -1
DAB_E_UNSUPPORTED = -6
DAB_LOSS_TRIVIAL = 0
DAB_LOSS_HUBER = 1
DAB_LOSS_SOFT_L1 = 2
DAB_LOSS_CAUCHY = 3
DAB_INTR_CENTER = 1
DAB_INTR_FOCAL = 2
DAB_INTR_DISTORTION = 4
DAB_EXT_ROTATION = 0x07
DAB_EXT_TRANSLATION = 0x38
DAB_SCHUR_PAIRS = 0
DAB_SCHUR_TILES = 1
DAB_SCHUR_DIRECT = 2
LOSS_KINDS = {"trivial": DAB_LOSS_TRIVIAL, "huber": DAB_LOSS_HUBER, "soft_l1": DAB_LOSS_SOFT_L1,
              "cauchy": DAB_LOSS_CAUCHY}


def loss_kind(kind):
    """DAB_LOSS_* of a loss given by name ("cauchy"), by number, or None (trivial)."""
    if kind is None:
        return DAB_LOSS_TRIVIAL
    if isinstance(kind, str):
        if kind.lower() not in LOSS_KINDS:
            raise ValueError(f"unknown loss {kind!r}: one of {sorted(LOSS_KINDS)}")
        return LOSS_KINDS[kind.lower()]
    return int(kind)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)


class DabProblem(C.Structure):
    _fields_ = [
        ("num_obs", C.c_int32), ("num_points", C.c_int32), ("num_ext", C.c_int32),
        ("num_intr", C.c_int32),
        ("obs_xy", _dp), ("obs_point", _ip), ("obs_ext0", _ip), ("obs_ext1", _ip),
        ("obs_intr", _ip), ("points", _dp), ("ext", _dp), ("intr", _dp),
        ("intr_nf", _ip), ("intr_nk", _ip), ("ext_const", _u8p),
        ("freeze_camera", C.c_int32), ("reserved", C.c_int32),
    ]


class DabOptions(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32), ("linear_solver_type", C.c_int32),
        ("max_solver_time_in_seconds", C.c_double), ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
        ("min_relative_decrease", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
        ("max_num_consecutive_invalid_steps", C.c_int32), ("jacobi_scaling", C.c_int32),
        ("minimizer_progress_to_stdout", C.c_int32), ("num_threads", C.c_int32),
        ("max_linear_solver_iterations", C.c_int32), ("min_linear_solver_iterations", C.c_int32),
        ("eta", C.c_double), ("pcg_fp32", C.c_int32), ("reserved", C.c_int32),
    ]


class DabIteration(C.Structure):
    _fields_ = [
        ("iteration", C.c_int32), ("step_is_successful", C.c_int32),
        ("step_is_valid", C.c_int32), ("linear_solver_iterations", C.c_int32),
        ("cost", C.c_double), ("cost_change", C.c_double), ("gradient_max_norm", C.c_double),
        ("step_norm", C.c_double), ("relative_decrease", C.c_double),
        ("trust_region_radius", C.c_double), ("iteration_time_in_seconds", C.c_double),
    ]


class DabSummary(C.Structure):
    _fields_ = [
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
        ("num_iterations", C.c_int32), ("num_successful_steps", C.c_int32),
        ("num_unsuccessful_steps", C.c_int32), ("termination_type", C.c_int32),
        ("num_residuals", C.c_int32), ("num_parameters", C.c_int32),
        ("num_free_points", C.c_int32), ("num_free_ext", C.c_int32),
        ("total_time_in_seconds", C.c_double),
        ("jacobian_evaluation_time_in_seconds", C.c_double),
        ("residual_evaluation_time_in_seconds", C.c_double),
        ("linear_solver_time_in_seconds", C.c_double),
        ("message", C.c_char * 256),
        ("iterations", C.POINTER(DabIteration)), ("iterations_capacity", C.c_int32),
        ("iterations_written", C.c_int32), ("linear_solver_type_used", C.c_int32),
        ("schur_assembly", C.c_int32),
    ]


class DabCovarianceOptions(C.Structure):
    _fields_ = [("min_pivot_ratio", C.c_double), ("jacobi_scaling", C.c_int32),
                ("reserved", C.c_int32)]


class DabCovarianceInfo(C.Structure):
    _fields_ = [
        ("status", C.c_int32), ("num_free_ext", C.c_int32), ("num_free_points", C.c_int32),
        ("first_deficient_point", C.c_int32), ("deficient_points", C.c_int32),
        ("schur_assembly", C.c_int32), ("point_pivot_ratio_min", C.c_double),
        ("camera_pivot_ratio", C.c_double), ("cost", C.c_double), ("num_residuals", C.c_int32),
        ("num_parameters", C.c_int32), ("evaluate_ms", C.c_double), ("factor_ms", C.c_double),
        ("inverse_ms", C.c_double), ("points_ms", C.c_double),
    ]


class DabCovarianceIntrInfo(C.Structure):
    _fields_ = [("num_free_intr", C.c_int32), ("num_free_scalars", C.c_int32),
                ("border_ms", C.c_double), ("reserved", C.c_double)]


class DabCovBlocksRequest(C.Structure):
    _fields_ = [("num_pp", C.c_int32), ("pp", _ip), ("num_pe", C.c_int32), ("pe", _ip),
                ("num_pz", C.c_int32), ("pz", _ip)]


COV_STATUS = {0: "OK", 1: "RANK_DEFICIENT"}


class DabSynthConfig(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("num_cameras", C.c_int32), ("num_arcs", C.c_int32),
        ("num_rings", C.c_int32), ("num_points", C.c_int32), ("obs_per_point", C.c_int32),
        ("seed", C.c_uint64), ("point_seed", C.c_uint64), ("pixel_noise", C.c_double),
        ("point_noise", C.c_double),
        ("rot_noise", C.c_double), ("trans_noise", C.c_double),
    ]


# int (*)(double* buf, int64_t count, int op, void* user): op 0 = sum, 1 = max
HostAllreduceFn = C.CFUNCTYPE(C.c_int, _dp, C.c_int64, C.c_int, C.c_void_p)

# name -> (restype, argtypes); every symbol include/dab.h declares
SIGNATURES = {
    "dab_abi_version": (C.c_int, []),
    "dab_last_error": (C.c_char_p, []),
    "dab_options_init": (None, [C.POINTER(DabOptions)]),
    "dab_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "dab_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "dab_create_dist": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_uint8),
                                  C.POINTER(C.c_void_p)]),
    "dab_create_dist_host": (C.c_int, [C.c_int, C.c_int, C.c_int, HostAllreduceFn, C.c_void_p,
                                       C.POINTER(C.c_void_p)]),
    "dab_destroy": (C.c_int, [C.c_void_p]),
    "dab_release_caches": (C.c_int, []),
    "dab_set_problem": (C.c_int, [C.c_void_p, C.POINTER(DabProblem)]),
    "dab_update_parameters": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_solve": (C.c_int, [C.c_void_p, C.POINTER(DabOptions), C.POINTER(DabSummary)]),
    "dab_set_loss": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "dab_get_loss": (C.c_int, [C.c_void_p, _ip, _dp]),
    "dab_get_parameters": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_set_intrinsics_free": (C.c_int, [C.c_void_p, _u8p]),
    "dab_get_intrinsics_free": (C.c_int, [C.c_void_p, _u8p, _ip, _ip]),
    "dab_set_points_constant": (C.c_int, [C.c_void_p, _u8p]),
    "dab_get_points_constant": (C.c_int, [C.c_void_p, _u8p, _ip]),
    "dab_set_ext_scalars_constant": (C.c_int, [C.c_void_p, _u8p]),
    "dab_get_ext_scalars_constant": (C.c_int, [C.c_void_p, _u8p, _ip]),
    "dab_set_ext_priors": (C.c_int, [C.c_void_p, C.c_int32, _ip, _dp, _dp]),
    "dab_get_ext_priors": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _dp, _dp]),
    "dab_eval_ext_priors": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_set_point_priors": (C.c_int, [C.c_void_p, C.c_int32, _ip, _dp, _dp]),
    "dab_get_point_priors": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _dp, _dp]),
    "dab_eval_point_priors": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_set_intr_priors": (C.c_int, [C.c_void_p, C.c_int32, _ip, _dp, _dp]),
    "dab_get_intr_priors": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _dp, _dp]),
    "dab_eval_intr_priors": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_get_intrinsics": (C.c_int, [C.c_void_p, _dp]),
    "dab_update_intrinsics": (C.c_int, [C.c_void_p, _dp]),
    "dab_eval_intrinsic_jacobians": (C.c_int, [C.c_void_p, _dp]),
    "dab_get_intrinsic_blocks": (C.c_int, [C.c_void_p, _ip, _dp]),
    "dab_covariance_options_init": (None, [C.POINTER(DabCovarianceOptions)]),
    "dab_covariance": (C.c_int, [C.c_void_p, C.POINTER(DabCovarianceOptions), _dp, _dp, _dp,
                                 C.POINTER(DabCovarianceInfo)]),
    "dab_covariance_intrinsics": (C.c_int, [C.c_void_p, C.POINTER(DabCovarianceOptions), _dp, _dp, _dp, _dp,
                                            C.POINTER(DabCovarianceInfo), C.POINTER(DabCovarianceIntrInfo)]),
    "dab_covariance_blocks": (C.c_int, [C.c_void_p, C.POINTER(DabCovarianceOptions), C.POINTER(DabCovBlocksRequest),
                                        _dp, _dp, _dp, C.POINTER(DabCovarianceInfo),
                                        C.POINTER(DabCovarianceIntrInfo), _dp]),
    "dab_eval_residuals": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_eval_jacobians": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_filter": (C.c_int, [C.c_void_p, C.c_double, _dp, C.c_double, _u8p, _u8p, _ip, _ip]),
    "dab_dense_spd_solve": (C.c_int, [C.c_void_p, C.c_int, _dp, _dp, _dp, _dp]),
    "dab_bench_eval_pass": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "dab_sync": (C.c_int, [C.c_void_p]),
    "dab_bench_get_blocks": (C.c_int, [C.c_void_p, _ip, _ip, _dp, _dp, _dp, _dp, _dp]),
    "dab_bench_kernel_ms": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_jacobian_bytes": (C.c_int, [C.c_void_p, _dp]),
    "dab_bench_pair_ms": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dab_eval_schedule": (C.c_int, [C.c_void_p, _ip]),
    "dab_pcg_schedule": (C.c_int, [C.c_void_p, _ip]),
    "dab_comm_schedule": (C.c_int, [C.c_void_p, _ip]),
    "dab_synth_sizes": (C.c_int, [C.POINTER(DabSynthConfig), _ip, _ip, _ip, _ip]),
    "dab_synth_fill": (C.c_int, [C.POINTER(DabSynthConfig), C.POINTER(DabProblem), _u8p]),
}

_LIB = None


def load_library(path=None):
    """Load libdab.so (the HIP build). Raises if it is missing: there is no fallback."""
    global _LIB
    if _LIB is not None and path is None:
        return _LIB
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"libdab.so not found at {p}: build it with `make -C deeparc-sfm_amd` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    if lib.dab_abi_version() != 2:
        raise RuntimeError("libdab ABI version mismatch")
    if path is None:
        _LIB = lib
    return lib


def last_error(lib=None):
    lib = lib or load_library()
    msg = lib.dab_last_error()
    return msg.decode() if msg else ""


def check(rc, lib=None):
    if rc != 0:
        raise RuntimeError(f"libdab error {rc}: {last_error(lib)}")
    return rc
