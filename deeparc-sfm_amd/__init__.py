"""deeparc-sfm_amd — MI355X-native bundle-adjustment hot path for pureexe/deeparc-sfm.

The product is libdab.so (gfx950 HIP kernels + C ABI, include/dab.h) plus the C++ host
adapter; this Python package is a thin ctypes mirror used by tests and bench.py.
Import it as ``deeparc_sfm_amd`` via _pkgload.load() (the directory name has a hyphen).
"""
from ._abi import (DAB_CONVERGENCE, DAB_E_INVALID, DAB_E_UNSUPPORTED, DAB_FAILURE, DAB_LINEAR_SOLVER_AUTO,
                   DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG, DAB_LOSS_CAUCHY,
                   DAB_LOSS_HUBER, DAB_LOSS_SOFT_L1, DAB_LOSS_TRIVIAL, DAB_NO_CONVERGENCE, LIB_PATH,
                   SIGNATURES, load_library, last_error)
from ._abi import DabCovBlocksRequest, DabCovarianceInfo, DabCovarianceIntrInfo, DabCovarianceOptions
from ._abi import DAB_INTR_CENTER, DAB_INTR_DISTORTION, DAB_INTR_FOCAL
from ._abi import DAB_EXT_ROTATION, DAB_EXT_TRANSLATION
from ._abi import DAB_SCHUR_DIRECT, DAB_SCHUR_PAIRS, DAB_SCHUR_TILES
from .core import (CONFIGS, Problem, Solver, covariance_options, options, point_sqrt_info_from_sigmas, solve,
                   sqrt_info_from_sigmas, synth, synth_config)

__all__ = [
    "CONFIGS", "Problem", "Solver", "options", "solve", "synth", "synth_config",
    "covariance_options", "DabCovarianceOptions", "DabCovarianceInfo", "DabCovarianceIntrInfo",
    "DabCovBlocksRequest",
    "load_library", "last_error", "LIB_PATH", "SIGNATURES",
    "DAB_CONVERGENCE", "DAB_NO_CONVERGENCE", "DAB_FAILURE",
    "DAB_LINEAR_SOLVER_EXPLICIT_SCHUR", "DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG", "DAB_LINEAR_SOLVER_AUTO",
    "DAB_LOSS_TRIVIAL", "DAB_LOSS_HUBER", "DAB_LOSS_SOFT_L1", "DAB_LOSS_CAUCHY",
    "DAB_E_INVALID", "DAB_E_UNSUPPORTED",
    "DAB_INTR_CENTER", "DAB_INTR_FOCAL", "DAB_INTR_DISTORTION",
    "DAB_EXT_ROTATION", "DAB_EXT_TRANSLATION",
    "DAB_SCHUR_PAIRS", "DAB_SCHUR_TILES", "DAB_SCHUR_DIRECT",
    "sqrt_info_from_sigmas", "point_sqrt_info_from_sigmas",
]
