"""ctypes binding of the host adapter (include/deeparc_host.h, libdeeparc_host.so).

The C++ adapter mirrors the reference's DeepArcManager (src/DeepArcManager.hh) and the
sfm.cc driver functions over libdab. This module exposes the same names to Python:
    m = DeepArcManager(); m.read(path); solve(m, 100, 3600, freeze_camera=True)
    m.filterPoint3d(5.0, center, radius); m.write(path); m.writePly(path)
    center, radius = fit_hemisphere(m.getCameraCenter())
The library raises RuntimeError when the reference would throw.
"""
import ctypes as C
import os

import numpy as np

from . import _abi

HOST_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libdeeparc_host.so")
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)

# dam_pipeline_report's breakdown fields, in order
PIPELINE_STAGES = ("read", "fit", "write", "marshal", "setup", "update", "prep", "lm", "writeback", "filter_device",
                   "filter_host")


class PipelineReport(C.Structure):  # dam_pipeline_report
    _fields_ = [("hemisphere_center", C.c_double * 3), ("hemisphere_radius", C.c_double),
                ("rounds", C.c_int32), ("final_blocks", C.c_int32), ("final_points", C.c_int32),
                ("solves", C.c_int32), ("lm_iterations", C.c_int32), ("reserved", C.c_int32),
                ("final_cost", C.c_double), ("solve_seconds", C.c_double), ("filter_seconds", C.c_double),
                ("total_seconds", C.c_double)] + [(k + "_seconds", C.c_double) for k in PIPELINE_STAGES]


SIGNATURES = {
    "dam_last_error": (C.c_char_p, []),
    "dam_create": (C.c_int, [C.POINTER(C.c_void_p)]),
    "dam_destroy": (C.c_int, [C.c_void_p]),
    "dam_read": (C.c_int, [C.c_void_p, C.c_char_p]),
    "dam_write": (C.c_int, [C.c_void_p, C.c_char_p]),
    "dam_write_ply": (C.c_int, [C.c_void_p, C.c_char_p]),
    "dam_sizes": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _ip, _ip, _ip, _ip]),
    "dam_get_points": (C.c_int, [C.c_void_p, _dp, _ip]),
    "dam_get_cameras": (C.c_int, [C.c_void_p, _dp, _dp]),
    "dam_get_blocks": (C.c_int, [C.c_void_p, _ip, _ip, _ip, _dp]),
    "dam_solve": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                            C.POINTER(_abi.DabSummary)]),
    "dam_set_loss": (C.c_int, [C.c_void_p, C.c_int32, C.c_double]),
    "dam_set_intrinsics_free": (C.c_int, [C.c_void_p, C.c_int32]),
    "dam_set_points_constant": (C.c_int, [C.c_void_p, C.c_int32]),
    "dam_set_ext_scalars_constant": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint8)]),
    "dam_set_ext_priors": (C.c_int, [C.c_void_p, C.c_int32, _ip, _dp, _dp]),
    "dam_set_point_priors": (C.c_int, [C.c_void_p, C.c_int32, _ip, _dp, _dp]),
    "dam_get_point_priors": (C.c_int, [C.c_void_p, _ip, _ip, _dp, _dp]),
    "dam_set_intr_priors": (C.c_int, [C.c_void_p, C.c_int32, _ip, _dp, _dp]),
    "dam_covariance": (C.c_int, [C.c_void_p, _ip, C.c_int32, C.c_int32, _dp, _dp, _dp, _ip,
                                 C.POINTER(_abi.DabCovarianceInfo)]),
    "dam_covariance_intrinsics": (C.c_int, [C.c_void_p, _ip, C.c_int32, _dp, _dp, _dp, _dp, _ip, _ip,
                                            C.POINTER(_abi.DabCovarianceInfo),
                                            C.POINTER(_abi.DabCovarianceIntrInfo)]),
    "dam_filter": (C.c_int, [C.c_void_p, C.c_double, _dp, C.c_double]),
    "dam_camera_centers": (C.c_int, [C.c_void_p, _dp, C.c_int32, _ip]),
    "dam_fit_hemisphere": (C.c_int, [_dp, C.c_int32, _dp, _dp, C.c_int32]),
    "dam_run_pipeline": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_double,
                                   _dp, _ip]),
    "dam_run_pipeline_report": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int32, C.c_int32, C.c_double,
                                          C.c_int32, C.POINTER(PipelineReport)]),
}

_LIB = None


def load_host_library():
    global _LIB
    if _LIB is None:
        _abi.load_library()  # libdab.so first (the host library links it)
        if not os.path.exists(HOST_LIB_PATH):
            raise RuntimeError(f"libdeeparc_host.so not found at {HOST_LIB_PATH}: run `make -C deeparc-sfm_amd`")
        lib = C.CDLL(HOST_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _LIB = lib
    return _LIB


def _check(rc):
    if rc != 0:
        raise RuntimeError(load_host_library().dam_last_error().decode())


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


class DeepArcManager:
    def __init__(self):
        self.lib = load_host_library()
        h = C.c_void_p()
        _check(self.lib.dam_create(C.byref(h)))
        self.h = h

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.dam_destroy(self.h)
            self.h = None

    def read(self, path):
        _check(self.lib.dam_read(self.h, os.fsencode(path)))
        return True

    def write(self, path):
        _check(self.lib.dam_write(self.h, os.fsencode(path)))

    def writePly(self, path):  # noqa: N802 (reference name)
        _check(self.lib.dam_write_ply(self.h, os.fsencode(path)))

    def sizes(self):
        v = [C.c_int32() for _ in range(7)]
        _check(self.lib.dam_sizes(self.h, *[C.byref(x) for x in v]))
        keys = ("blocks", "points", "intrinsics", "extrinsics", "shared", "arc", "ring")
        return dict(zip(keys, [x.value for x in v]))

    def isShareExtrinsic(self):  # noqa: N802
        return bool(self.sizes()["shared"])

    def points(self):
        n = self.sizes()["points"]
        xyz, rgb = np.zeros((n, 3)), np.zeros((n, 3), np.int32)
        _check(self.lib.dam_get_points(self.h, _p(xyz, C.c_double), _p(rgb, C.c_int32)))
        return xyz, rgb

    def cameras(self):
        s = self.sizes()
        ext, intr = np.zeros((s["extrinsics"], 6)), np.zeros((s["intrinsics"], 6))
        _check(self.lib.dam_get_cameras(self.h, _p(ext, C.c_double), _p(intr, C.c_double)))
        return ext, intr

    def blocks(self):
        n = self.sizes()["blocks"]
        a, r, pi = (np.zeros(n, np.int32) for _ in range(3))
        xy = np.zeros((n, 2))
        _check(self.lib.dam_get_blocks(self.h, _p(a, C.c_int32), _p(r, C.c_int32), _p(pi, C.c_int32),
                                       _p(xy, C.c_double)))
        return a, r, pi, xy

    def getCameraCenter(self):  # noqa: N802
        n = C.c_int32()
        _check(self.lib.dam_camera_centers(self.h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3))
        _check(self.lib.dam_camera_centers(self.h, _p(out, C.c_double), n.value, C.byref(n)))
        return out

    def set_loss(self, kind, scale=1.0):
        """Robust loss of every later solve() of this manager (dam_set_loss): kind as
        core.Solver.set_loss, e.g. set_loss("cauchy", 0.5) for `new ceres::CauchyLoss(0.5)`."""
        _check(self.lib.dam_set_loss(self.h, _abi.loss_kind(kind), float(scale)))

    def set_intrinsics_free(self, groups):
        """Intrinsic groups (DAB_INTR_* bits) every later solve() of this manager refines
        (dam_set_intrinsics_free): the equivalent of deleting sfm.cc:60-62. cameras() and write()
        see the refined values."""
        _check(self.lib.dam_set_intrinsics_free(self.h, int(groups)))

    def set_points_constant(self, all_points=True):
        """Every later solve() of this manager holds all points constant (dam_set_points_constant):
        the reference's commented-out sfm.cc:59; False frees them again."""
        _check(self.lib.dam_set_points_constant(self.h, int(bool(all_points))))

    def set_ext_scalars_constant(self, bits):
        """Every later solve() of this manager holds these scalars of the extrinsics constant
        (dam_set_ext_scalars_constant; core.Solver.set_ext_scalars_constant's argument, indexed as
        cameras()' extrinsics): one int for every extrinsic or one byte each; None clears it."""
        if bits is None:
            _check(self.lib.dam_set_ext_scalars_constant(self.h, None))
            return
        ne = self.sizes()["extrinsics"]
        b = np.asarray(bits)
        if b.ndim == 0:
            b = np.full(ne, int(b))
        if b.shape != (ne,) or (b < 0).any() or (b > 255).any():
            raise ValueError(f"bits: one int or {ne} values in 0..63")
        b = np.ascontiguousarray(b, np.uint8)
        _check(self.lib.dam_set_ext_scalars_constant(self.h, _p(b, C.c_uint8)))

    def set_ext_priors(self, index, mean=None, sqrt_info=None):
        """Gaussian priors on extrinsics for every later solve() of this manager
        (dam_set_ext_priors; core.Solver.set_ext_priors' arguments, index in extrinsics()); None or
        an empty index clears them."""
        if index is None or np.size(index) == 0:
            _check(self.lib.dam_set_ext_priors(self.h, 0, None, None, None))
            return
        idx = np.ascontiguousarray(index, np.int32).reshape(-1)
        n = idx.shape[0]
        mu = np.ascontiguousarray(mean, np.float64)
        a = np.ascontiguousarray(sqrt_info, np.float64)
        if mu.shape != (n, 6) or a.shape != (n, 6, 6):
            raise ValueError(f"mean: ({n}, 6) and sqrt_info: ({n}, 6, 6) values")
        _check(self.lib.dam_set_ext_priors(self.h, n, _p(idx, C.c_int32), _p(mu, C.c_double), _p(a, C.c_double)))

    def set_point_priors(self, index, mean=None, sqrt_info=None):
        """Gaussian priors on points for every later solve() of this manager
        (dam_set_point_priors; core.Solver.set_point_priors' arguments, index into points()); None
        or an empty index clears them. filterPoint3d renumbers them with the point list."""
        if index is None or np.size(index) == 0:
            _check(self.lib.dam_set_point_priors(self.h, 0, None, None, None))
            return
        idx = np.ascontiguousarray(index, np.int32).reshape(-1)
        n = idx.shape[0]
        mu = np.ascontiguousarray(mean, np.float64)
        a = np.ascontiguousarray(sqrt_info, np.float64)
        if mu.shape != (n, 3) or a.shape != (n, 3, 3):
            raise ValueError(f"mean: ({n}, 3) and sqrt_info: ({n}, 3, 3) values")
        _check(self.lib.dam_set_point_priors(self.h, n, _p(idx, C.c_int32), _p(mu, C.c_double), _p(a, C.c_double)))

    def set_intr_priors(self, index, mean=None, sqrt_info=None):
        """Gaussian priors on intrinsics for every later solve() of this manager
        (dam_set_intr_priors; core.Solver.set_intr_priors' arguments, index in intrinsics()); None
        or an empty index clears them."""
        if index is None or np.size(index) == 0:
            _check(self.lib.dam_set_intr_priors(self.h, 0, None, None, None))
            return
        idx = np.ascontiguousarray(index, np.int32).reshape(-1)
        n = idx.shape[0]
        mu = np.ascontiguousarray(mean, np.float64)
        a = np.ascontiguousarray(sqrt_info, np.float64)
        if mu.shape != (n, 6) or a.shape != (n, 6, 6):
            raise ValueError(f"mean: ({n}, 6) and sqrt_info: ({n}, 6, 6) values")
        _check(self.lib.dam_set_intr_priors(self.h, n, _p(idx, C.c_int32), _p(mu, C.c_double), _p(a, C.c_double)))

    def get_point_priors(self):
        """(index [n], mean [n][3], sqrt_info [n][3][3]) as the manager holds them now."""
        n = C.c_int32()
        _check(self.lib.dam_get_point_priors(self.h, C.byref(n), None, None, None))
        idx, mu, a = np.zeros(n.value, np.int32), np.zeros((n.value, 3)), np.zeros((n.value, 3, 3))
        _check(self.lib.dam_get_point_priors(self.h, None, _p(idx, C.c_int32), _p(mu, C.c_double), _p(a, C.c_double)))
        return idx, mu, a

    def covariance(self, extra_const=(), freeze_camera=False, full=False):
        """DeepArcManager::covariance (dam_covariance): the covariance of the current scene at its
        current parameters under the manager's loss, shaped like core.Solver.covariance: `info`,
        `point_cov` (points, 3, 3) in points() order, `ext_cov` (nfe, 6, 6) with `ext_index` and
        `ext_label` rows ("arc" | "ring", position), `ext_full` when full. extra_const: extrinsic
        indices held constant beside the gauge rule's (one more fixes the rig's scale gauge);
        the arrays are None when info["status"] is "RANK_DEFICIENT"."""
        from .core import _unpack_sym
        ex = np.ascontiguousarray(list(extra_const), np.int32)
        info = _abi.DabCovarianceInfo()

        def call(pc, ec, ef, lab):
            _check(self.lib.dam_covariance(self.h, _p(ex, C.c_int32) if ex.size else None, int(ex.size),
                                           int(bool(freeze_camera)), pc, ec, ef, lab, C.byref(info)))
        call(None, None, None, None)
        d = {k: getattr(info, k) for k, _ in _abi.DabCovarianceInfo._fields_}
        d["status"] = _abi.COV_STATUS.get(info.status, str(info.status))
        if info.status != 0:
            return dict(info=d, point_cov=None, ext_cov=None, ext_index=None, ext_label=None, ext_full=None)
        nfe, npts = info.num_free_ext, self.sizes()["points"]
        pc, ec = np.zeros((npts, 6)), np.zeros((nfe, 21))
        ef = np.zeros((6 * nfe, 6 * nfe)) if full else None
        lab = np.zeros((nfe, 3), np.int32)
        call(_p(pc, C.c_double), _p(ec, C.c_double), _p(ef, C.c_double) if full else None, _p(lab, C.c_int32))
        return dict(info=d, point_cov=_unpack_sym(pc, 3), ext_cov=_unpack_sym(ec, 6), ext_index=lab[:, 0].copy(),
                    ext_label=[("ring" if k else "arc", int(p)) for _, k, p in lab], ext_full=ef)

    def covariance_intrinsics(self, extra_const=(), full=False):
        """DeepArcManager::covarianceIntrinsics (dam_covariance_intrinsics): covariance() with the
        groups of set_intrinsics_free as unknowns, shaped like core.Solver.covariance(intrinsics=
        True): also `intr_cov` (nfi, 6, 6), `intr_index` and `cam_full` when full."""
        from .core import _unpack_sym
        ex = np.ascontiguousarray(list(extra_const), np.int32)
        info, zinfo = _abi.DabCovarianceInfo(), _abi.DabCovarianceIntrInfo()

        def call(pc, ec, zc, cf, lab, zi):
            _check(self.lib.dam_covariance_intrinsics(self.h, _p(ex, C.c_int32) if ex.size else None, int(ex.size),
                                                      pc, ec, zc, cf, lab, zi, C.byref(info), C.byref(zinfo)))
        call(None, None, None, None, None, None)
        d = {k: getattr(info, k) for k, _ in _abi.DabCovarianceInfo._fields_}
        d.update(num_free_intr=zinfo.num_free_intr, num_free_scalars=zinfo.num_free_scalars)
        d["status"] = _abi.COV_STATUS.get(info.status, str(info.status))
        if info.status != 0:
            return dict(info=d, point_cov=None, ext_cov=None, ext_index=None, ext_label=None, intr_cov=None,
                        intr_index=None, cam_full=None)
        nfe, nfi, npts = info.num_free_ext, zinfo.num_free_intr, self.sizes()["points"]
        pc, ec, zc = np.zeros((npts, 6)), np.zeros((nfe, 21)), np.zeros((nfi, 21))
        cf = np.zeros((6 * nfe + 6 * nfi, 6 * nfe + 6 * nfi)) if full else None
        lab, zi = np.zeros((nfe, 3), np.int32), np.zeros(nfi, np.int32)
        call(_p(pc, C.c_double), _p(ec, C.c_double), _p(zc, C.c_double), _p(cf, C.c_double) if full else None,
             _p(lab, C.c_int32), _p(zi, C.c_int32))
        return dict(info=d, point_cov=_unpack_sym(pc, 3), ext_cov=_unpack_sym(ec, 6), ext_index=lab[:, 0].copy(),
                    ext_label=[("ring" if k else "arc", int(p)) for _, k, p in lab], intr_cov=_unpack_sym(zc, 6),
                    intr_index=zi, cam_full=cf)

    def filterPoint3d(self, error_boundary, hemisphere_center, hemisphere_radius):  # noqa: N802
        c = np.ascontiguousarray(hemisphere_center, np.float64)
        _check(self.lib.dam_filter(self.h, float(error_boundary), _p(c, C.c_double), float(hemisphere_radius)))


def solve(manager, max_iteration=1000, max_second=3600, freeze_camera=False,
          linear_solver_type=_abi.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR):
    """sfm.cc:31 solve() on the GPU; returns the summary as a dict."""
    from .core import summary_to_dict
    its = (_abi.DabIteration * 1024)()
    s = _abi.DabSummary()
    s.iterations = C.cast(its, C.POINTER(_abi.DabIteration))
    s.iterations_capacity = 1024
    _check(manager.lib.dam_solve(manager.h, int(max_iteration), int(max_second), int(bool(freeze_camera)),
                                 int(linear_solver_type), C.byref(s)))
    return summary_to_dict(s, its)


def fit_hemisphere(centers, center=(0.0, 0.0, 0.0), radius=1.0, max_iteration=1000):
    lib = load_host_library()
    P = np.ascontiguousarray(centers, np.float64).reshape(-1, 3)
    c = np.array(center, np.float64)
    r = C.c_double(radius)
    _check(lib.dam_fit_hemisphere(_p(P, C.c_double), P.shape[0], _p(c, C.c_double), C.byref(r), max_iteration))
    return c, r.value


def run_pipeline(input_path, output_path="", ply_prefix="", max_iteration=100, max_second=3600,
                 error_boundary=5.0):
    """sfm.cc main(): fit, freeze-camera solve, filter, then solve + filter to a fixed point."""
    lib = load_host_library()
    hemi = np.zeros(4)
    counts = np.zeros(3, np.int32)
    _check(lib.dam_run_pipeline(os.fsencode(input_path), os.fsencode(output_path), os.fsencode(ply_prefix),
                                max_iteration, max_second, error_boundary, _p(hemi, C.c_double),
                                _p(counts, C.c_int32)))
    return dict(hemisphere_center=hemi[:3].copy(), hemisphere_radius=float(hemi[3]), rounds=int(counts[0]),
                blocks=int(counts[1]), points=int(counts[2]))


def run_pipeline_report(input_path, output_path="", ply_prefix="", max_iteration=100, max_second=3600,
                        error_boundary=5.0, quiet=True):
    """run_pipeline with the full report (solves, LM iterations, last cost, host timings);
    quiet suppresses the reference's per-iteration progress lines."""
    lib = load_host_library()
    r = PipelineReport()
    _check(lib.dam_run_pipeline_report(os.fsencode(input_path), os.fsencode(output_path), os.fsencode(ply_prefix),
                                       max_iteration, max_second, error_boundary, 1 if quiet else 0, C.byref(r)))
    return dict(hemisphere_center=np.array(r.hemisphere_center[:]), hemisphere_radius=r.hemisphere_radius,
                rounds=r.rounds, blocks=r.final_blocks, points=r.final_points, solves=r.solves,
                lm_iterations=r.lm_iterations, final_cost=r.final_cost, solve_seconds=r.solve_seconds,
                filter_seconds=r.filter_seconds, total_seconds=r.total_seconds,
                breakdown={k: getattr(r, k + "_seconds") for k in PIPELINE_STAGES})
