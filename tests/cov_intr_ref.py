"""TEST INFRASTRUCTURE ONLY: the arrays of dab_covariance_intrinsics from a dense Sigma (a plain
module).

Sigma = (J^T J)^-1 over the referenced points, the free extrinsics and the active intrinsic
scalars (lm_ref.Layout: the scalars dab_solve counts), J from lm_ref.jacobian. Sigma is
cov_ref.sigma_inv of that Jacobian, pinned against cov_ref.sigma_pinv by
tests/test_cov_intr_ref.py, and split by blocks() into the arrays of the call: inactive slots (the
model lacks them or the mask leaves them out) get zero rows and columns; without a free scalar
cam_full is dab_covariance's ext_full. kappa is that of the Jacobi-scaled H over all columns; the
rank test is cov_ref.rank_test with the z columns beside the cameras'. Also the cases the CPU and
GPU tests share.
"""
from types import SimpleNamespace

import numpy as np

import cov_ref as cr
import intr_ref as ir
import robust_ref as rr


def free_intrinsics(L):
    """Indices of the free intrinsics (some active scalar), ascending."""
    return np.flatnonzero(L.act.any(axis=1)).astype(np.int32)


def blocks(Sigma, L, prob):
    """The arrays of dab_covariance_intrinsics from the dense Sigma: point_cov (num_points, 3, 3)
    with NaN rows for unreferenced points, ext_cov (nc, 6, 6), intr_cov (nfi, 6, 6), cam_full
    (6 nc + 6 nfi square: extrinsics, then the six slots of every free intrinsic), ext_index,
    intr_index, active (nfi, 6) bool."""
    npts = prob.points.shape[0]
    pc = np.full((npts, 3, 3), np.nan)
    for i, p in enumerate(L.pt_of):
        pc[p] = Sigma[3 * i:3 * i + 3, 3 * i:3 * i + 3]
    n3 = 3 * L.np
    free = free_intrinsics(L)
    nfi = len(free)
    n2 = 6 * L.nc + 6 * nfi
    # where each column of Sigma's camera part lands in cam_full
    dst = np.concatenate([np.arange(6 * L.nc),
                          np.array([6 * L.nc + 6 * int(np.searchsorted(free, i)) + k for i, k in zip(L.zi, L.zk)],
                                   np.int64)]).astype(np.int64)
    full = np.zeros((n2, n2))
    full[np.ix_(dst, dst)] = Sigma[n3:, n3:]
    ec = np.stack([full[6 * c:6 * c + 6, 6 * c:6 * c + 6] for c in range(L.nc)]) if L.nc else np.zeros((0, 6, 6))
    o = 6 * L.nc
    zc = (np.stack([full[o + 6 * i:o + 6 * i + 6, o + 6 * i:o + 6 * i + 6] for i in range(nfi)]) if nfi
          else np.zeros((0, 6, 6)))
    return dict(point_cov=pc, ext_cov=ec, intr_cov=zc, cam_full=full, ext_index=L.ext_of.astype(np.int32),
                intr_index=free, active=L.act[free])


def rank_test(A, L, thr=cr.MIN_PIVOT_RATIO):
    """cov_ref.rank_test with the active intrinsic columns beside the cameras' in the reduced system."""
    return cr.rank_test(A, SimpleNamespace(np=L.np, nc=L.nc + int(L.nz > 0)), thr)


def bound(ref):
    """The accuracy bound of every returned array: 64 kappa 2^-53 max |Sigma_ref| over the blocks."""
    m = max(np.nanmax(np.abs(ref["point_cov"])), np.abs(ref["cam_full"]).max() if ref["cam_full"].size else 0.0)
    return 64.0 * ref["kappa"] * cr.EPS * m, m


# ---- the shared cases -----------------------------------------------------------------------
def mixed(prob):
    """intr_nf = [1, 2, 1, 2, ...], intr_nk = [2, 1, 0, 2, 1, 0, ...], then the miscalibration of
    intr_ref: inactive slots, one focal length driving both rows, distortion on composed rows."""
    ni = prob.intr.shape[0]
    prob.intr_nf[:] = np.array([1, 2] * ni)[:ni]
    prob.intr_nk[:] = np.array([2, 1, 0] * ni)[:ni]
    return ir.offset_intrinsics(prob)


def first(prob, k, groups=7):
    """Groups on the intrinsics 0 .. k - 1 only."""
    g = np.zeros(prob.intr.shape[0], np.int64)
    g[:k] = groups
    return g


CASES = {
    "rig3x5": lambda pkg: (cr.rig3x5(pkg), 7),
    "rig6x20": lambda pkg: (cr.rig6x20(pkg), 7),
    "rig6x20-mixed": lambda pkg: (mixed(cr.rig6x20(pkg)), 7),
    "rig6x20-mixed-masks": lambda pkg: (mixed(cr.rig6x20(pkg)), np.array([7, 0, 2, 5, 0, 4])),
    "rig3x5-mixed": lambda pkg: (mixed(cr.rig3x5(pkg)), 7),
    "bal40-first16": lambda pkg: (lambda p: (p, first(p, 16)))(cr.bal40(pkg)),
    "bal170-first16": lambda pkg: (lambda p: (p, first(p, 16)))(cr.bal170(pkg)),
    "bal40-ragged-first16": lambda pkg: (lambda p: (p, first(p, 16)))(cr.bal40_ragged(pkg)),
    "rig6x20-focal": lambda pkg: (cr.rig6x20(pkg), 2),
    "bal40-first16-focal": lambda pkg: (lambda p: (p, first(p, 16, 2)))(cr.bal40(pkg)),
}
# active scalars and n' = (6 free extrinsics, 6 free intrinsics) of every case
SIZES = {"rig3x5": (12, 30, 18), "rig6x20": (24, 138, 36), "rig6x20-mixed": (27, 138, 36),
         "rig6x20-mixed-masks": (10, 138, 18), "rig3x5-mixed": (13, 30, 18), "bal40-first16": (80, 228, 96),
         "bal170-first16": (80, 1008, 96), "bal40-ragged-first16": (80, 228, 96), "rig6x20-focal": (12, 138, 36),
         "bal40-first16-focal": (16, 228, 96)}
LOSSES = {"huber": (rr.HUBER, 1.0), "cauchy": (rr.CAUCHY, 2.0)}
