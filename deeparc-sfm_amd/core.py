"""Python host mirror of the reference BA interface over the C ABI (libdab.so).

Mirrors (names, argument meaning, error behaviour) of the reference:
  solve(manager_or_problem, max_iteration=1000, max_second=3600, freeze_camera=False)
      src/sfm.cc:31-75 — builds the problem from the observation -> parameter mapping
      (ParameterBlock::get(), ParameterBlock.hh:68-94), applies the gauge / constancy
      rules (sfm.cc:50-63) and solves with the DENSE_SCHUR-equivalent solver
      (sfm.cc:66-73). Parameters are updated in place, as Ceres does.
  Problem.residuals()   — SnavelyReprojectionError::operator()(double) per observation
      (DeepArcManager.cc:335-346)
The heavy lifting is the gfx950 HIP library; this module only marshals numpy arrays.
"""
import ctypes as C

import numpy as np

from . import _abi
from ._abi import (DabOptions, DabProblem, DabSummary, DabIteration, DabSynthConfig,
                   DabCovarianceOptions, DabCovarianceInfo, DabCovarianceIntrInfo, check, load_library)


def _ptr(a, ct):
    return a.ctypes.data_as(C.POINTER(ct)) if a is not None else None


class Problem:
    """SoA bundle-adjustment problem (the dab_problem of include/dab.h) backed by numpy."""

    def __init__(self, obs_xy, obs_point, obs_ext0, obs_ext1, obs_intr, points, ext, intr,
                 intr_nf, intr_nk, ext_const=None, freeze_camera=False):
        self.obs_xy = np.ascontiguousarray(obs_xy, dtype=np.float64).reshape(-1, 2)
        self.obs_point = np.ascontiguousarray(obs_point, dtype=np.int32)
        self.obs_ext0 = np.ascontiguousarray(obs_ext0, dtype=np.int32)
        self.obs_ext1 = np.ascontiguousarray(obs_ext1, dtype=np.int32)
        self.obs_intr = np.ascontiguousarray(obs_intr, dtype=np.int32)
        self.points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self.ext = np.ascontiguousarray(ext, dtype=np.float64).reshape(-1, 6)
        self.intr = np.ascontiguousarray(intr, dtype=np.float64).reshape(-1, 6)
        self.intr_nf = np.ascontiguousarray(intr_nf, dtype=np.int32)
        self.intr_nk = np.ascontiguousarray(intr_nk, dtype=np.int32)
        self.ext_const = (np.ascontiguousarray(ext_const, dtype=np.uint8)
                          if ext_const is not None else None)
        self.freeze_camera = bool(freeze_camera)

    @property
    def num_obs(self):
        return int(self.obs_point.shape[0])

    def copy(self):
        return Problem(self.obs_xy.copy(), self.obs_point.copy(), self.obs_ext0.copy(),
                       self.obs_ext1.copy(), self.obs_intr.copy(), self.points.copy(),
                       self.ext.copy(), self.intr.copy(), self.intr_nf.copy(),
                       self.intr_nk.copy(),
                       None if self.ext_const is None else self.ext_const.copy(),
                       self.freeze_camera)

    def subset(self, obs_mask):
        """Observations selected by obs_mask; parameter arrays are shared (not copied)."""
        m = np.asarray(obs_mask)
        return Problem(self.obs_xy[m], self.obs_point[m], self.obs_ext0[m], self.obs_ext1[m],
                       self.obs_intr[m], self.points, self.ext, self.intr, self.intr_nf,
                       self.intr_nk, self.ext_const, self.freeze_camera)

    def point_owner(self, world):
        """Owner rank of every point for a world-size sharding (partition by
        point, so V, V^-1 and the back-substitution stay GPU-local): contiguous point-id
        ranges whose observation counts are balanced. Cameras are replicated."""
        npts = int(self.points.shape[0])
        cnt = np.bincount(self.obs_point, minlength=npts).astype(np.int64)
        total = int(cnt.sum())
        start = np.cumsum(cnt) - cnt
        return np.minimum(start * world // max(total, 1), world - 1).astype(np.int32)

    def shard(self, rank, world):
        """The observations of the points owned by `rank` (parameter arrays shared, the
        gauge / ext_const of the global problem kept)."""
        if world <= 1:
            return self
        owner = self.point_owner(world)
        return self.subset(owner[self.obs_point] == rank)

    def shard_point_priors(self, point_priors, rank, world):
        """The part of a global point-prior set (index, mean, sqrt_info) that belongs to `rank`:
        the priors on the points that rank owns (point ids are global on a shard). What that rank
        passes to Solver.set_point_priors on the handle of shard(rank, world)."""
        idx, mu, a = point_priors
        idx = np.asarray(idx, np.int32).reshape(-1)
        mu = np.asarray(mu, np.float64).reshape(-1, 3)
        a = np.asarray(a, np.float64).reshape(-1, 3, 3)
        if world <= 1:
            return idx, mu, a
        keep = self.point_owner(world)[idx] == rank
        return idx[keep], mu[keep], a[keep]

    def as_c(self):
        """dab_problem view of the arrays (valid while self is alive)."""
        p = DabProblem()
        p.num_obs = self.num_obs
        p.num_points = int(self.points.shape[0])
        p.num_ext = int(self.ext.shape[0])
        p.num_intr = int(self.intr.shape[0])
        p.obs_xy = _ptr(self.obs_xy, C.c_double)
        p.obs_point = _ptr(self.obs_point, C.c_int32)
        p.obs_ext0 = _ptr(self.obs_ext0, C.c_int32)
        p.obs_ext1 = _ptr(self.obs_ext1, C.c_int32)
        p.obs_intr = _ptr(self.obs_intr, C.c_int32)
        p.points = _ptr(self.points, C.c_double)
        p.ext = _ptr(self.ext, C.c_double)
        p.intr = _ptr(self.intr, C.c_double)
        p.intr_nf = _ptr(self.intr_nf, C.c_int32)
        p.intr_nk = _ptr(self.intr_nk, C.c_int32)
        p.ext_const = _ptr(self.ext_const, C.c_uint8) if self.ext_const is not None else None
        p.freeze_camera = int(self.freeze_camera)
        return p


def synth_config(kind=0, num_cameras=0, num_arcs=0, num_rings=0, num_points=0,
                 obs_per_point=10, seed=1, point_seed=0, pixel_noise=1.0, point_noise=0.01,
                 rot_noise=1e-3, trans_noise=1e-3):
    c = DabSynthConfig()
    c.kind, c.num_cameras, c.num_arcs, c.num_rings = kind, num_cameras, num_arcs, num_rings
    c.num_points, c.obs_per_point, c.seed, c.point_seed = num_points, obs_per_point, seed, point_seed
    c.pixel_noise, c.point_noise, c.rot_noise, c.trans_noise = (pixel_noise, point_noise,
                                                                rot_noise, trans_noise)
    return c


def synth(**kw):
    """Deterministic synthetic problem generated by libdab's host code."""
    lib = load_library()
    cfg = synth_config(**kw)
    no, npt, ne, ni = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    check(lib.dab_synth_sizes(C.byref(cfg), C.byref(no), C.byref(npt), C.byref(ne),
                              C.byref(ni)), lib)
    no, npt, ne, ni = no.value, npt.value, ne.value, ni.value
    pr = Problem(np.zeros((no, 2)), np.zeros(no, np.int32), np.zeros(no, np.int32),
                 np.zeros(no, np.int32), np.zeros(no, np.int32), np.zeros((npt, 3)),
                 np.zeros((ne, 6)), np.zeros((ni, 6)), np.zeros(ni, np.int32),
                 np.zeros(ni, np.int32), np.zeros(ne, np.uint8))
    cp = pr.as_c()
    check(lib.dab_synth_fill(C.byref(cfg), C.byref(cp), _ptr(pr.ext_const, C.c_uint8)), lib)
    return pr


# SURVEY §8d named configurations
CONFIGS = {
    "c1_rig_8x36": dict(kind=1, num_arcs=8, num_rings=36, num_points=20000, obs_per_point=8, seed=4),
    "c2_100cam": dict(kind=0, num_cameras=100, num_points=10000, obs_per_point=10, seed=1),
    "c3_1kcam": dict(kind=0, num_cameras=1000, num_points=100000, obs_per_point=10, seed=2),
    "c5_rig_16x64": dict(kind=1, num_arcs=16, num_rings=64, num_points=1000000,
                         obs_per_point=10, seed=3),
}


def options(**kw):
    lib = load_library()
    o = DabOptions()
    lib.dab_options_init(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(f"unknown option {k}")
        setattr(o, k, v)
    return o


def covariance_options(**kw):
    """dab_covariance_options with the library's defaults (min_pivot_ratio 1e-10,
    jacobi_scaling 1), then the given fields."""
    lib = load_library()
    o = DabCovarianceOptions()
    lib.dab_covariance_options_init(C.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise AttributeError(f"unknown option {k}")
        setattr(o, k, v)
    return o


def _unpack_sym(a, n):
    """[m][n (n + 1) / 2] upper-packed rows -> [m][n][n] symmetric."""
    iu = np.triu_indices(n)
    out = np.zeros((a.shape[0], n, n))
    out[:, iu[0], iu[1]] = a
    out[:, iu[1], iu[0]] = a
    return out


def summary_to_dict(s, its):
    return dict(
        initial_cost=s.initial_cost, final_cost=s.final_cost, num_iterations=s.num_iterations,
        num_successful_steps=s.num_successful_steps,
        num_unsuccessful_steps=s.num_unsuccessful_steps,
        termination=_abi.TERMINATION.get(s.termination_type, str(s.termination_type)),
        message=s.message.decode(errors="replace"), num_residuals=s.num_residuals,
        num_parameters=s.num_parameters, num_free_points=s.num_free_points,
        num_free_ext=s.num_free_ext, total_time=s.total_time_in_seconds,
        jacobian_time=s.jacobian_evaluation_time_in_seconds,
        residual_time=s.residual_evaluation_time_in_seconds,
        linear_solver_time=s.linear_solver_time_in_seconds,
        linear_solver_type_used=s.linear_solver_type_used, schur_assembly=s.schur_assembly,
        iterations=[dict(iteration=it.iteration, success=bool(it.step_is_successful),
                         valid=bool(it.step_is_valid), cost=it.cost, cost_change=it.cost_change,
                         gradient_max_norm=it.gradient_max_norm, step_norm=it.step_norm,
                         relative_decrease=it.relative_decrease,
                         trust_region_radius=it.trust_region_radius,
                         linear_solver_iterations=it.linear_solver_iterations,
                         time=it.iteration_time_in_seconds)
                    for it in its[: s.iterations_written]])


class Solver:
    """One libdab handle (one GPU). For multi-GPU pass rank/world/unique_id (RCCL).

    host_allreduce (rehearsal only): a callable(np.ndarray, op) that all-reduces the array
    in place across ranks (op "sum" | "max"), e.g. over gloo; the library then stages its
    collectives through host memory instead of RCCL, so several ranks may share one GPU."""

    def __init__(self, device=0, rank=0, world_size=1, unique_id=None, host_allreduce=None):
        self.lib = load_library()
        h = C.c_void_p()
        self._cb = None
        if world_size > 1 and host_allreduce is not None:
            def _cb(buf, count, op, user):
                try:
                    arr = np.ctypeslib.as_array(buf, shape=(int(count),))
                    host_allreduce(arr, "max" if op == 1 else "sum")
                    return 0
                except Exception:  # reported to the library as a collective failure
                    return 1
            self._cb = _abi.HostAllreduceFn(_cb)
            check(self.lib.dab_create_dist_host(device, rank, world_size, self._cb, None, C.byref(h)),
                  self.lib)
        elif world_size > 1 or unique_id is not None:
            # world_size 1 with a unique id: a one-rank RCCL communicator, every collective
            # executed (the multi-GPU transport rehearsed on one GPU)
            buf = (C.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
            check(self.lib.dab_create_dist(device, rank, world_size, buf, C.byref(h)), self.lib)
        else:
            check(self.lib.dab_create(device, C.byref(h)), self.lib)
        self.h = h
        self.problem = None
        self._cp = None
        self._intr_free = False

    @staticmethod
    def unique_id():
        lib = load_library()
        buf = (C.c_uint8 * 128)()
        check(lib.dab_comm_unique_id(buf), lib)
        return bytes(buf)

    def close(self):
        if self.h:
            self.lib.dab_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_problem(self, problem):
        self.problem = problem
        self._cp = problem.as_c()
        check(self.lib.dab_set_problem(self.h, C.byref(self._cp)), self.lib)
        self._intr_free = False  # dab_set_problem resets the mask

    def update_parameters(self, points=None, ext=None):
        check(self.lib.dab_update_parameters(
            self.h, _ptr(np.ascontiguousarray(points, np.float64), C.c_double) if points is not None else None,
            _ptr(np.ascontiguousarray(ext, np.float64), C.c_double) if ext is not None else None), self.lib)

    def set_loss(self, kind, scale=1.0):
        """Robust loss of every observation (dab_set_loss): kind "trivial" | "huber" | "soft_l1" |
        "cauchy" (or a DAB_LOSS_* number, or None = trivial), scale = Ceres' `a`. State of the
        handle: it survives set_problem and holds for every later solve until set again."""
        check(self.lib.dab_set_loss(self.h, _abi.loss_kind(kind), float(scale)), self.lib)

    def get_loss(self):
        """(kind name, scale) of the handle's loss; ("trivial", 0.0) when none is set."""
        k, a = C.c_int32(), C.c_double()
        check(self.lib.dab_get_loss(self.h, C.byref(k), C.byref(a)), self.lib)
        names = {v: n for n, v in _abi.LOSS_KINDS.items()}
        return names[k.value], a.value

    def set_intrinsics_free(self, groups):
        """Which intrinsic groups the next solve refines (dab_set_intrinsics_free): DAB_INTR_*
        bits (CENTER 1 | FOCAL 2 | DISTORTION 4), one int for every intrinsic or an array of
        num_intr; 0 / None = all constant. Set after set_problem, which resets it."""
        ni = int(self.problem.intr.shape[0])
        if groups is None:
            check(self.lib.dab_set_intrinsics_free(self.h, None), self.lib)
            self._intr_free = False
            return
        g = np.asarray(groups)
        if g.ndim == 0:
            g = np.full(ni, int(g))
        if g.shape != (ni,) or (g < 0).any() or (g > 255).any():
            raise ValueError(f"groups: one int or {ni} values in 0..7")
        g = np.ascontiguousarray(g, np.uint8)
        check(self.lib.dab_set_intrinsics_free(self.h, _ptr(g, C.c_uint8)), self.lib)
        self._intr_free = bool(g.any())

    def get_intrinsics_free(self):
        """(groups [num_intr] uint8, free intrinsics, free scalars) of the mask on the handle."""
        g = np.zeros(int(self.problem.intr.shape[0]), np.uint8)
        nfi, ns = C.c_int32(), C.c_int32()
        check(self.lib.dab_get_intrinsics_free(self.h, _ptr(g, C.c_uint8), C.byref(nfi), C.byref(ns)), self.lib)
        return g, nfi.value, ns.value

    def set_points_constant(self, mask):
        """Which points the next solve and covariance hold constant (dab_set_points_constant, the
        reference's commented-out sfm.cc:59): True / a non-zero scalar for every point, False /
        0 / None for none, or an array of num_points (any non-zero entry = constant). Set after
        set_problem, which resets it; it survives update_parameters and set_loss."""
        npts = int(self.problem.points.shape[0])
        if mask is None or (np.ndim(mask) == 0 and not mask):
            check(self.lib.dab_set_points_constant(self.h, None), self.lib)
            return
        m = np.asarray(mask)
        if m.ndim == 0:
            m = np.full(npts, True)
        if m.shape != (npts,):
            raise ValueError(f"mask: a bool or {npts} values")
        m = np.ascontiguousarray(m != 0, np.uint8)
        check(self.lib.dab_set_points_constant(self.h, _ptr(m, C.c_uint8)), self.lib)

    def get_points_constant(self):
        """(mask [num_points] uint8 as set, points of this rank both referenced and constant)."""
        m = np.zeros(int(self.problem.points.shape[0]), np.uint8)
        n = C.c_int32()
        check(self.lib.dab_get_points_constant(self.h, _ptr(m, C.c_uint8), C.byref(n)), self.lib)
        return m, n.value

    def set_ext_scalars_constant(self, bits):
        """Which scalars of each extrinsic the next solve and covariance hold constant
        (dab_set_ext_scalars_constant): bit k = scalar k of (w0,w1,w2,t0,t1,t2), DAB_EXT_ROTATION
        7 | DAB_EXT_TRANSLATION 56, one int for every extrinsic or an array of num_ext; 0 / None =
        none. Set after set_problem, which resets it; it survives every other setter. Bits on a
        constant or unreferenced extrinsic are ignored."""
        ne = int(self.problem.ext.shape[0])
        if bits is None:
            check(self.lib.dab_set_ext_scalars_constant(self.h, None), self.lib)
            return
        b = np.asarray(bits)
        if b.ndim == 0:
            b = np.full(ne, int(b))
        if b.shape != (ne,) or (b < 0).any() or (b > 255).any():
            raise ValueError(f"bits: one int or {ne} values in 0..63")
        b = np.ascontiguousarray(b, np.uint8)
        check(self.lib.dab_set_ext_scalars_constant(self.h, _ptr(b, C.c_uint8)), self.lib)

    def get_ext_scalars_constant(self):
        """(bits [num_ext] uint8 as set, effective constant scalars: those on free extrinsics)."""
        b = np.zeros(int(self.problem.ext.shape[0]), np.uint8)
        n = C.c_int32()
        check(self.lib.dab_get_ext_scalars_constant(self.h, _ptr(b, C.c_uint8), C.byref(n)), self.lib)
        return b, n.value

    def set_ext_priors(self, index, mean=None, sqrt_info=None):
        """Gaussian priors on extrinsics (dab_set_ext_priors; Ceres' NormalPrior(A, mu) with a NULL
        loss on the extrinsic's block): index [n] extrinsic indices, mean [n][6] in the library's
        (w, t), sqrt_info [n][6][6] = A of the residual A (x - mean). None or an empty index
        clears them. Set after set_problem, which resets them; they survive update_parameters,
        set_loss and the masks. A prior on a constant or unreferenced extrinsic is ignored."""
        if index is None or np.size(index) == 0:
            check(self.lib.dab_set_ext_priors(self.h, 0, None, None, None), self.lib)
            return
        idx = np.ascontiguousarray(index, np.int32).reshape(-1)
        n = idx.shape[0]
        mu = np.ascontiguousarray(mean, np.float64)
        a = np.ascontiguousarray(sqrt_info, np.float64)
        if mu.shape != (n, 6) or a.shape != (n, 6, 6):
            raise ValueError(f"mean: ({n}, 6) and sqrt_info: ({n}, 6, 6) values")
        check(self.lib.dab_set_ext_priors(self.h, n, _ptr(idx, C.c_int32), _ptr(mu, C.c_double),
                                          _ptr(a, C.c_double)), self.lib)

    def get_ext_priors(self):
        """(index [n], mean [n][6], sqrt_info [n][6][6], num_effective) as set."""
        n, ne = C.c_int32(), C.c_int32()
        check(self.lib.dab_get_ext_priors(self.h, C.byref(n), C.byref(ne), None, None, None), self.lib)
        idx = np.zeros(n.value, np.int32)
        mu = np.zeros((n.value, 6))
        a = np.zeros((n.value, 6, 6))
        check(self.lib.dab_get_ext_priors(self.h, None, None, _ptr(idx, C.c_int32), _ptr(mu, C.c_double),
                                          _ptr(a, C.c_double)), self.lib)
        return idx, mu, a, ne.value

    def eval_ext_priors(self):
        """(residuals [n][6] in the order set, cost = 0.5 sum |r|^2 over the effective priors) at
        the parameters on the handle (dab_eval_ext_priors); an ignored prior's row is zero."""
        n = C.c_int32()
        check(self.lib.dab_get_ext_priors(self.h, C.byref(n), None, None, None, None), self.lib)
        r = np.zeros((n.value, 6))
        cost = C.c_double()
        check(self.lib.dab_eval_ext_priors(self.h, _ptr(r, C.c_double), C.byref(cost)), self.lib)
        return r, cost.value

    def set_point_priors(self, index, mean=None, sqrt_info=None):
        """Gaussian priors on points (dab_set_point_priors; Ceres' NormalPrior(A, mu) with a NULL
        loss on the point's block): index [n] point ids, mean [n][3], sqrt_info [n][3][3] = A of the
        residual A (X - mean). None or an empty index clears them. Set after set_problem, which
        resets them; they survive update_parameters, set_loss, the masks and set_ext_priors. A
        prior on a constant or unreferenced point is ignored. On a multi-rank handle each rank
        sets the priors of its own shard's points (Problem.shard_point_priors)."""
        if index is None or np.size(index) == 0:
            check(self.lib.dab_set_point_priors(self.h, 0, None, None, None), self.lib)
            return
        idx = np.ascontiguousarray(index, np.int32).reshape(-1)
        n = idx.shape[0]
        mu = np.ascontiguousarray(mean, np.float64)
        a = np.ascontiguousarray(sqrt_info, np.float64)
        if mu.shape != (n, 3) or a.shape != (n, 3, 3):
            raise ValueError(f"mean: ({n}, 3) and sqrt_info: ({n}, 3, 3) values")
        check(self.lib.dab_set_point_priors(self.h, n, _ptr(idx, C.c_int32), _ptr(mu, C.c_double),
                                            _ptr(a, C.c_double)), self.lib)

    def get_point_priors(self):
        """(index [n], mean [n][3], sqrt_info [n][3][3], num_effective) as set."""
        n, ne = C.c_int32(), C.c_int32()
        check(self.lib.dab_get_point_priors(self.h, C.byref(n), C.byref(ne), None, None, None), self.lib)
        idx = np.zeros(n.value, np.int32)
        mu = np.zeros((n.value, 3))
        a = np.zeros((n.value, 3, 3))
        check(self.lib.dab_get_point_priors(self.h, None, None, _ptr(idx, C.c_int32), _ptr(mu, C.c_double),
                                            _ptr(a, C.c_double)), self.lib)
        return idx, mu, a, ne.value

    def eval_point_priors(self):
        """(residuals [n][3] in the order set, cost = 0.5 sum |r|^2 over this rank's effective
        priors) at the parameters on the handle (dab_eval_point_priors); an ignored prior's row
        is zero."""
        n = C.c_int32()
        check(self.lib.dab_get_point_priors(self.h, C.byref(n), None, None, None, None), self.lib)
        r = np.zeros((n.value, 3))
        cost = C.c_double()
        check(self.lib.dab_eval_point_priors(self.h, _ptr(r, C.c_double), C.byref(cost)), self.lib)
        return r, cost.value

    def set_intr_priors(self, index, mean=None, sqrt_info=None):
        """Gaussian priors on intrinsics (dab_set_intr_priors; Ceres' NormalPrior(A, mu) with a NULL
        loss over the intrinsic's three blocks): index [n] intrinsic indices, mean [n][6] in
        Problem.intr's slots (cx, cy, f0, f1, k0, k1), sqrt_info [n][6][6] = A of the residual
        A (x - mean). None or an empty index clears them. Set after set_problem, which resets them;
        they survive update_parameters, update_intrinsics, set_loss, the masks and the other
        priors. Slots the model lacks or the mask leaves constant take no part; a prior on an
        intrinsic outside the free set (set_intrinsics_free) is ignored. On a multi-rank handle
        every rank sets the same priors."""
        if index is None or np.size(index) == 0:
            check(self.lib.dab_set_intr_priors(self.h, 0, None, None, None), self.lib)
            return
        idx = np.ascontiguousarray(index, np.int32).reshape(-1)
        n = idx.shape[0]
        mu = np.ascontiguousarray(mean, np.float64)
        a = np.ascontiguousarray(sqrt_info, np.float64)
        if mu.shape != (n, 6) or a.shape != (n, 6, 6):
            raise ValueError(f"mean: ({n}, 6) and sqrt_info: ({n}, 6, 6) values")
        check(self.lib.dab_set_intr_priors(self.h, n, _ptr(idx, C.c_int32), _ptr(mu, C.c_double),
                                           _ptr(a, C.c_double)), self.lib)

    def get_intr_priors(self):
        """(index [n], mean [n][6], sqrt_info [n][6][6], num_effective) as set."""
        n, ne = C.c_int32(), C.c_int32()
        check(self.lib.dab_get_intr_priors(self.h, C.byref(n), C.byref(ne), None, None, None), self.lib)
        idx = np.zeros(n.value, np.int32)
        mu = np.zeros((n.value, 6))
        a = np.zeros((n.value, 6, 6))
        check(self.lib.dab_get_intr_priors(self.h, None, None, _ptr(idx, C.c_int32), _ptr(mu, C.c_double),
                                           _ptr(a, C.c_double)), self.lib)
        return idx, mu, a, ne.value

    def eval_intr_priors(self):
        """(residuals [n][6] in the order set, cost = 0.5 sum |r|^2 over the effective priors) at
        the intrinsics on the handle (dab_eval_intr_priors); an ignored prior's row is zero."""
        n = C.c_int32()
        check(self.lib.dab_get_intr_priors(self.h, C.byref(n), None, None, None, None), self.lib)
        r = np.zeros((n.value, 6))
        cost = C.c_double()
        check(self.lib.dab_eval_intr_priors(self.h, _ptr(r, C.c_double), C.byref(cost)), self.lib)
        return r, cost.value

    def get_intrinsics(self):
        """The intrinsics on the handle, [num_intr][6] (refined ones after a solve)."""
        k = np.zeros((int(self.problem.intr.shape[0]), 6))
        check(self.lib.dab_get_intrinsics(self.h, _ptr(k, C.c_double)), self.lib)
        return k

    def update_intrinsics(self, intr):
        k = np.ascontiguousarray(intr, np.float64).reshape(-1, 6)
        if k.shape[0] != self.problem.intr.shape[0]:
            raise ValueError("intr: [num_intr][6]")
        check(self.lib.dab_update_intrinsics(self.h, _ptr(k, C.c_double)), self.lib)

    def intrinsic_jacobians(self):
        """d r / d (cx, cy, f0, f1, k0, k1) per observation, (num_obs, 2, 6), raw."""
        J = np.zeros((self.problem.num_obs, 2, 6))
        check(self.lib.dab_eval_intrinsic_jacobians(self.h, _ptr(J, C.c_double)), self.lib)
        return J

    def intrinsic_blocks(self):
        """[U_zz upper 21 | g_z 6] per free intrinsic of the last evaluation (nfi, 27)."""
        n = C.c_int32()
        check(self.lib.dab_get_intrinsic_blocks(self.h, C.byref(n), None), self.lib)
        zg = np.zeros((n.value, 27))
        if n.value:
            check(self.lib.dab_get_intrinsic_blocks(self.h, C.byref(n), _ptr(zg, C.c_double)), self.lib)
        return zg

    def solve(self, opts=None, max_records=1024):
        o = opts if opts is not None else options()
        its = (DabIteration * max_records)()
        s = DabSummary()
        s.iterations = C.cast(its, C.POINTER(DabIteration))
        s.iterations_capacity = max_records
        check(self.lib.dab_solve(self.h, C.byref(o), C.byref(s)), self.lib)
        # dab_problem.intr is const for the library: the refined values are copied here, in place
        # like points and ext (identical to the problem's own when no intrinsic is free)
        if self._intr_free:
            self.problem.intr[...] = self.get_intrinsics()
        return summary_to_dict(s, its)

    def covariance(self, points=True, ext=True, full=False, intrinsics=False, **opts):
        """Sigma = (J^T J)^-1 at the parameters on the handle (dab_covariance; no sigma^2 factor:
        multiply by 2 info["cost"] / (num_residuals - num_parameters)). Returns a dict with
        `info`, `point_cov` (num_points, 3, 3) with NaN rows for unreferenced points, `ext_cov`
        (nfe, 6, 6) with `ext_index` (the extrinsic of each block; None on a shard whose free set
        is a union over ranks), and `ext_full` (6 nfe, 6 nfe) when full. When info["status"] is
        "RANK_DEFICIENT" the arrays are None: drop single-observation points (Problem.subset) or
        fix the scale gauge with a constant point (set_points_constant) or one more constant
        extrinsic. Two library calls: the size and
        rank query, then the arrays.

        intrinsics=True: the free intrinsics of set_intrinsics_free are unknowns as well
        (dab_covariance_intrinsics; the default call refuses a handle with a non-empty free set).
        The dict gains `intr_cov` (nfi, 6, 6) over the slots (cx, cy, f0, f1, k0, k1) with zero
        rows and columns for inactive slots, `intr_index` (the intrinsic of each block; None on a
        shard whose referenced set is a union over ranks), `cam_full` (6 nfe + 6 nfi square:
        extrinsics, then intrinsics) when full, and info's num_free_intr, num_free_scalars and
        border_ms."""
        if intrinsics:
            return self._covariance_intrinsics(points, ext, full, opts)
        o = covariance_options(**opts)
        info = DabCovarianceInfo()
        check(self.lib.dab_covariance(self.h, C.byref(o), None, None, None, C.byref(info)), self.lib)
        nfe, npts = info.num_free_ext, int(self.problem.points.shape[0])
        pc = np.zeros((npts, 6)) if points else None
        ec = np.zeros((nfe, 21)) if ext else None
        ef = np.zeros((6 * nfe, 6 * nfe)) if full else None
        if info.status == 0 and (points or ext or full):
            check(self.lib.dab_covariance(self.h, C.byref(o), _ptr(pc, C.c_double), _ptr(ec, C.c_double),
                                          _ptr(ef, C.c_double), C.byref(info)), self.lib)
        d = {k: getattr(info, k) for k, _ in DabCovarianceInfo._fields_}
        d["status"] = _abi.COV_STATUS.get(info.status, str(info.status))
        ok = info.status == 0
        pr = self.problem
        idx = None
        if not pr.freeze_camera:
            used = np.unique(np.concatenate([pr.obs_ext0, pr.obs_ext1[pr.obs_ext1 >= 0]]))
            if pr.ext_const is not None:
                used = used[pr.ext_const[used] == 0]
            idx = used.astype(np.int32) if used.shape[0] == nfe else None
        elif nfe == 0:
            idx = np.zeros(0, np.int32)
        return dict(info=d, point_cov=_unpack_sym(pc, 3) if ok and points else None,
                    ext_cov=_unpack_sym(ec, 6) if ok and ext else None, ext_index=idx,
                    ext_full=ef if ok and full else None)

    def _ext_index(self, nfe):
        pr = self.problem
        if pr.freeze_camera:
            return np.zeros(0, np.int32) if nfe == 0 else None
        used = np.unique(np.concatenate([pr.obs_ext0, pr.obs_ext1[pr.obs_ext1 >= 0]]))
        if pr.ext_const is not None:
            used = used[pr.ext_const[used] == 0]
        return used.astype(np.int32) if used.shape[0] == nfe else None

    def _intr_index(self, nfi):
        """The intrinsic of each block of intr_cov: referenced, with an active scalar selected."""
        pr = self.problem
        groups = self.get_intrinsics_free()[0].astype(np.int64)
        if pr.freeze_camera:
            groups[:] = 0
        has = np.stack([groups & 1, groups & 1, groups & 2, (groups & 2) * (pr.intr_nf == 2),
                        (groups & 4) * (pr.intr_nk >= 1), (groups & 4) * (pr.intr_nk >= 2)], axis=1) != 0
        ref = np.zeros(groups.shape[0], bool)
        ref[pr.obs_intr] = True
        idx = np.flatnonzero(has.any(axis=1) & ref).astype(np.int32)
        return idx if idx.shape[0] == nfi else None

    def _covariance_intrinsics(self, points, ext, full, opts):
        o = covariance_options(**opts)
        info, zinfo = DabCovarianceInfo(), DabCovarianceIntrInfo()
        call = self.lib.dab_covariance_intrinsics
        check(call(self.h, C.byref(o), None, None, None, None, C.byref(info), C.byref(zinfo)), self.lib)
        nfe, nfi, npts = info.num_free_ext, zinfo.num_free_intr, int(self.problem.points.shape[0])
        n2 = 6 * nfe + 6 * nfi
        pc = np.zeros((npts, 6)) if points else None
        ec = np.zeros((nfe, 21)) if ext else None
        zc = np.zeros((nfi, 21))
        cf = np.zeros((n2, n2)) if full else None
        if info.status == 0:
            check(call(self.h, C.byref(o), _ptr(pc, C.c_double), _ptr(ec, C.c_double), _ptr(zc, C.c_double),
                       _ptr(cf, C.c_double), C.byref(info), C.byref(zinfo)), self.lib)
        d = {k: getattr(info, k) for k, _ in DabCovarianceInfo._fields_}
        d.update({k: getattr(zinfo, k) for k in ("num_free_intr", "num_free_scalars", "border_ms")})
        d["status"] = _abi.COV_STATUS.get(info.status, str(info.status))
        ok = info.status == 0
        return dict(info=d, point_cov=_unpack_sym(pc, 3) if ok and points else None,
                    ext_cov=_unpack_sym(ec, 6) if ok and ext else None, ext_index=self._ext_index(nfe),
                    intr_cov=_unpack_sym(zc, 6) if ok else None, intr_index=self._intr_index(nfi),
                    cam_full=cf if ok and full else None)

    def covariance_blocks(self, pp=None, pe=None, pz=None, **opts):
        """Cross blocks of Sigma for lists of pairs (dab_covariance_blocks): `pp` (n, 2) point ids
        (a, b), `pe` (n, 2) (point id, extrinsic index), `pz` (n, 2) (point id, intrinsic index).
        Sigma is covariance()'s on a handle without free intrinsics and covariance(intrinsics=
        True)'s on one with them. Returns a dict with `info` (as covariance() returns it, with
        num_free_intr, num_free_scalars, border_ms and blocks_ms, the device time of the
        cross-block kernels) and `pp` (n, 3, 3), `pe` (n, 3, 6) over (w0, w1, w2, t0, t1, t2), `pz`
        (n, 3, 6) over (cx, cy, f0, f1, k0, k1); None for a list that was not given and for all
        three when info["status"] is "RANK_DEFICIENT". Blocks known exactly (a constant point, a
        constant extrinsic or scalar, an intrinsic or slot that is not free) are 0, blocks without
        information (a point this handle does not reference) NaN.

        The variance of the distance between the points a and b:

            c = s.covariance(ext=False)["point_cov"]
            x = s.covariance_blocks(pp=[(a, b)])["pp"][0]
            u = (X[a] - X[b]) / np.linalg.norm(X[a] - X[b])
            var = u @ (c[a] + c[b] - x - x.T) @ u        # times 2 cost / dof for sigma^2
        """
        o = covariance_options(**opts)
        info, zinfo = DabCovarianceInfo(), DabCovarianceIntrInfo()
        req = _abi.DabCovBlocksRequest()
        keep, outs = [], {}
        for name, width in (("pp", 9), ("pe", 18), ("pz", 18)):
            lst = {"pp": pp, "pe": pe, "pz": pz}[name]
            if lst is None:
                outs[name] = None
                continue
            idx = np.ascontiguousarray(np.asarray(lst, np.int32).reshape(-1, 2))
            keep.append(idx)
            outs[name] = np.zeros((idx.shape[0], width))
            setattr(req, "num_" + name, idx.shape[0])
            setattr(req, name, _ptr(idx, C.c_int32))
        ms = C.c_double(0.0)
        check(self.lib.dab_covariance_blocks(self.h, C.byref(o), C.byref(req), _ptr(outs["pp"], C.c_double),
                                             _ptr(outs["pe"], C.c_double), _ptr(outs["pz"], C.c_double),
                                             C.byref(info), C.byref(zinfo), C.byref(ms)), self.lib)
        d = {k: getattr(info, k) for k, _ in DabCovarianceInfo._fields_}
        d.update({k: getattr(zinfo, k) for k in ("num_free_intr", "num_free_scalars", "border_ms")})
        d["blocks_ms"] = ms.value
        d["status"] = _abi.COV_STATUS.get(info.status, str(info.status))
        ok = info.status == 0
        shape = {"pp": (3, 3), "pe": (3, 6), "pz": (3, 6)}
        res = {k: (v.reshape((-1,) + shape[k]) if ok and v is not None else None) for k, v in outs.items()}
        res["info"] = d
        return res

    def residuals(self):
        r = np.zeros((self.problem.num_obs, 2))
        cost = C.c_double()
        check(self.lib.dab_eval_residuals(self.h, _ptr(r, C.c_double), C.byref(cost)), self.lib)
        return r, cost.value

    def jacobians(self):
        n = self.problem.num_obs
        r = np.zeros((n, 2))
        J = np.zeros((n, 2, 15))
        check(self.lib.dab_eval_jacobians(self.h, _ptr(r, C.c_double), _ptr(J, C.c_double)),
              self.lib)
        return r, J

    def filter(self, error_boundary, center, radius):
        """filterPoint3d's masks on the resident problem (dab_filter): (observation keep,
        point keep) in the caller's order, uint8."""
        ok = np.zeros(self.problem.num_obs, np.uint8)
        pk = np.zeros(self.problem.points.shape[0], np.uint8)
        c = np.ascontiguousarray(center, np.float64)
        check(self.lib.dab_filter(self.h, float(error_boundary), _ptr(c, C.c_double), float(radius),
                                  _ptr(ok, C.c_uint8), _ptr(pk, C.c_uint8), None, None), self.lib)
        return ok, pk

    def get_parameters(self, points, ext):
        check(self.lib.dab_get_parameters(self.h, _ptr(points, C.c_double), _ptr(ext, C.c_double)),
              self.lib)

    def dense_spd_solve(self, A, b):
        """Solve A x = b with the library's device Cholesky. Returns (x, ms, ok)."""
        A = np.ascontiguousarray(A, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        x = np.zeros(b.shape[0])
        ms = C.c_double()
        rc = self.lib.dab_dense_spd_solve(self.h, int(b.shape[0]), _ptr(A, C.c_double),
                                          _ptr(b, C.c_double), _ptr(x, C.c_double), C.byref(ms))
        if rc < 0:
            check(rc, self.lib)
        return x, ms.value, rc == 0

    # --- benchmark hooks ---
    def bench_eval_pass(self, with_assembly=True, count=1):
        """Enqueue `count` evaluation passes (asynchronous; sync() waits)."""
        check(self.lib.dab_bench_eval_pass(self.h, int(with_assembly), int(count)), self.lib)

    def sync(self):
        check(self.lib.dab_sync(self.h), self.lib)

    def bench_blocks(self):
        """What the last evaluation pass computed (dab_bench_get_blocks): V [points][6],
        g [points][3], ug [free ext][27], ux [cross][36] and the cost."""
        nc, nx = C.c_int32(), C.c_int32()
        check(self.lib.dab_bench_get_blocks(self.h, C.byref(nc), C.byref(nx), None, None, None, None, None),
              self.lib)
        npts = self.problem.points.shape[0]
        V, g = np.zeros((npts, 6)), np.zeros((npts, 3))
        ug, ux = np.zeros((nc.value, 27)), np.zeros((nx.value, 36))
        cost = C.c_double()
        check(self.lib.dab_bench_get_blocks(self.h, None, None, _ptr(V, C.c_double), _ptr(g, C.c_double),
                                            _ptr(ug, C.c_double), _ptr(ux, C.c_double), C.byref(cost)), self.lib)
        return {"V": V, "g": g, "ug": ug, "ux": ux, "cost": np.array([cost.value])}

    def bench_kernel_ms(self):
        a, b = C.c_double(), C.c_double()
        check(self.lib.dab_bench_kernel_ms(self.h, C.byref(a), C.byref(b)), self.lib)
        return a.value, b.value

    def jacobian_bytes(self):
        b = C.c_double()
        check(self.lib.dab_jacobian_bytes(self.h, C.byref(b)), self.lib)
        return b.value

    def bench_pair_ms(self):
        """(ms per launch, algorithmic bytes per launch) of the rig's pair-major camera kernel
        over the batches read by the last bench_kernel_ms() call"""
        a, b = C.c_double(), C.c_double()
        check(self.lib.dab_bench_pair_ms(self.h, C.byref(a), C.byref(b)), self.lib)
        return a.value, b.value

    def comm_p2p(self):
        """1 when the one-shot xGMI peer-to-peer all-reduce carries the sums over ranks"""
        f = C.c_int32()
        check(self.lib.dab_comm_schedule(self.h, C.byref(f)), self.lib)
        return int(f.value)

    def pcg_matrix_free(self):
        """0: stored-Y products; 1: matrix-free fp64; 2: matrix-free mixed precision (pcg_fp32)"""
        f = C.c_int32()
        check(self.lib.dab_pcg_schedule(self.h, C.byref(f)), self.lib)
        return int(f.value)

    def eval_fused(self):
        f = C.c_int32()
        check(self.lib.dab_eval_schedule(self.h, C.byref(f)), self.lib)
        return f.value  # 0 two kernels, 1 one fused launch, 2 fused kernel split per side


def sqrt_info_from_sigmas(sigma_w, sigma_t, n=None):
    """sqrt_info of independent priors: diag(1 / sigma_w x3, 1 / sigma_t x3), one 6x6 or [n] of
    them. np.inf (or None) as a sigma gives zero rows: sqrt_info_from_sigmas(None, 0.01) is a
    position-only prior."""
    def inv(sg):
        return 0.0 if sg is None or np.isinf(sg) else 1.0 / float(sg)
    a = np.diag([inv(sigma_w)] * 3 + [inv(sigma_t)] * 3)
    return a if n is None else np.repeat(a[None], int(n), axis=0)


def point_sqrt_info_from_sigmas(sigma, n=None):
    """sqrt_info of independent point priors: diag(1 / sigma), sigma a scalar or one value per axis,
    one 3x3 or [n] of them. np.inf (or None) as a sigma gives a zero row:
    point_sqrt_info_from_sigmas((np.inf, np.inf, 0.01)) is height-only control."""
    sg = [sigma] * 3 if sigma is None or np.ndim(sigma) == 0 else list(sigma)
    if len(sg) != 3:
        raise ValueError("sigma: a scalar or 3 values")
    a = np.diag([0.0 if v is None or np.isinf(v) else 1.0 / float(v) for v in sg])
    return a if n is None else np.repeat(a[None], int(n), axis=0)


def solve(problem, max_iteration=1000, max_second=3600, freeze_camera=False, device=0,
          verbose=False, loss=None, free_intrinsics=0, freeze_points=False, ext_priors=None, point_priors=None,
          intr_priors=None, ext_scalars_constant=None, **opt_kw):
    """Drop-in for the reference's solve() (src/sfm.cc:31): DENSE_SCHUR-equivalent LM,
    max_num_iterations / max_solver_time_in_seconds as given, parameters updated in place.
    loss: None (the reference's NULL loss, sfm.cc:48) or a (kind, scale) pair such as
    ("cauchy", 0.5), the `new ceres::CauchyLoss(0.5)` the reference keeps commented out.
    free_intrinsics: DAB_INTR_* bits (an int or one per intrinsic) refined with the cameras, the
    equivalent of deleting sfm.cc:60-62; problem.intr is updated in place.
    freeze_points: True (every point) or a mask of num_points: the points held constant, the
    `SetParameterBlockConstant(parameter_block[0]); //freeze point3d` the reference keeps
    commented out at sfm.cc:59 (pose-only refinement, ground-control points).
    ext_priors: None or (index, mean, sqrt_info), Gaussian priors on extrinsics
    (Solver.set_ext_priors; sqrt_info_from_sigmas builds the diagonal case).
    point_priors: None or (index, mean, sqrt_info), Gaussian priors on points, applied after
    freeze_points (Solver.set_point_priors; point_sqrt_info_from_sigmas builds the diagonal case).
    intr_priors: None or (index, mean, sqrt_info), Gaussian priors on the intrinsics that
    free_intrinsics frees (Solver.set_intr_priors: a calibration with its covariance).
    ext_scalars_constant: None, or DAB_EXT_* bits (an int or one per extrinsic): the scalars of
    the free extrinsics held constant (Solver.set_ext_scalars_constant), the equivalent of
    keeping only one of sfm.cc:51-52 or of a SubsetManifold."""
    problem.freeze_camera = bool(freeze_camera)
    o = options(max_num_iterations=max_iteration, max_solver_time_in_seconds=float(max_second),
                minimizer_progress_to_stdout=int(verbose), **opt_kw)
    s = Solver(device)
    try:
        if loss is not None:
            s.set_loss(*loss)
        s.set_problem(problem)
        if np.any(np.asarray(free_intrinsics)):
            s.set_intrinsics_free(free_intrinsics)
        if np.any(np.asarray(freeze_points)):
            s.set_points_constant(freeze_points)
        if ext_scalars_constant is not None:
            s.set_ext_scalars_constant(ext_scalars_constant)
        if ext_priors is not None:
            s.set_ext_priors(*ext_priors)
        if point_priors is not None:
            s.set_point_priors(*point_priors)
        if intr_priors is not None:
            s.set_intr_priors(*intr_priors)
        return s.solve(o)
    finally:
        s.close()
