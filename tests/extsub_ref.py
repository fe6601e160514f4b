"""TEST INFRASTRUCTURE ONLY: the reference of the constant-extrinsic-scalar tests (a plain module).

dab_set_ext_scalars_constant holds single scalars of an extrinsic (w0,w1,w2,t0,t1,t2) constant:
one of sfm.cc:51-52 kept, or Ceres' SubsetManifold. The reference is lm_ref with the constant
scalars' columns absent from the layout: SubLayout is lm_ref.Layout without them, so x_norm,
gradient_max_norm, the Jacobi scale, the LM diagonal and num_parameters run over the free scalars
only, while num_free_ext and the camera order stay. A prior on an extrinsic keeps all six values in
its residual A (x_e - mu); only the free scalars' columns of A are rows of the Jacobian.

tests/lm_ref.py is frozen, so lm / jacobian run lm_ref's own loop with SubLayout (and the prior
rows over its columns) bound into that module for the duration of the call; folding the mask into
lm_ref.Layout is the follow-up. covariance puts exact-zero rows and columns back for the constant
scalars (known exactly), so its arrays have the shapes of dab_covariance(_intrinsics).

Here are also the cases and masks the CPU and GPU tests share. The reference's own spread between
two listings of the observations (given order and intr_ref.reorder), 25 iterations, measured by
tests/test_extsub_ref.py::test_two_observation_orders_agree (relative cost | ext | points):
  Blow rot-odd   3.5e-13 | 4.3e-13 | 2.6e-13  (4 iterations)
  Blow trans-all 3.3e-13 | 8.5e-13 | 8.5e-14  (25, 10 rejected)
  Blow mix       2.9e-16 | 2.0e-14 | 5.0e-16  (25, 5 rejected)
  R rot-odd      1.2e-12 | 2.0e-12 | 1.3e-12  (7)
  R trans-all    3.6e-14 | 2.2e-16 | 2.5e-16  (10)
  R mix          2.7e-14 | 1.6e-15 | 4.7e-16  (17, 4 rejected)
and under Cauchy(2.0), 15 iterations: Blow mix 6.7e-16 | 7.1e-15 | 1.9e-14, R trans-all
3.3e-15 | 3.3e-14 | 2.4e-14. The largest is 80 times under the bounds of that test (1e-10 of the
cost, 1e-9 of the parameters).
"""
from contextlib import contextmanager

import numpy as np

import cov_intr_ref as czr
import cov_ref as cr
import lm_ref as lr
import ptconst_ref as pr
import robust_ref as rr

ROTATION, TRANSLATION = 0x07, 0x38


def as_bits(prob, bits):
    """[num_ext] int from None / an int / an array of bytes in 0..63."""
    ne = prob.ext.shape[0]
    if bits is None:
        return np.zeros(ne, np.int64)
    b = np.asarray(bits, np.int64)
    if b.ndim == 0:
        b = np.full(ne, int(b), np.int64)
    assert b.shape == (ne,) and (b >= 0).all() and (b <= 63).all()
    return b


class SubLayout(lr.Layout):
    """lm_ref.Layout without the columns of the constant scalars of the free extrinsics. keep: the
    columns of the full layout that stay, in order; n_full: the full layout's width. np, nc, nz,
    pt_of, ext_of are the full layout's (the camera set does not change); n and n_pc shrink."""

    def __init__(self, prob, const=None, groups=0, bits=None):
        super().__init__(prob, const, groups)
        b = as_bits(prob, bits)[self.ext_of]
        self.ext_free = ((b[:, None] >> np.arange(6)) & 1) == 0  # [nc][6]
        keep = np.ones(self.n, bool)
        keep[3 * self.np:self.n_pc] = self.ext_free.ravel()
        self.keep = np.flatnonzero(keep)
        self.n_full, self.n_pc_full = self.n, self.n_pc
        self.n_sub = self.n_full - len(self.keep)
        new = -np.ones(self.n_full + 1, np.int64)  # [-1] stays -1
        new[self.keep] = np.arange(len(self.keep))
        self.col = new[self.col]
        self.zcol = new[self.zcol]
        self.n = len(self.keep)
        self.n_pc = self.n - self.nz

    def _pack_full(self, prob):
        return np.concatenate([prob.points[self.pt_of].ravel(), prob.ext[self.ext_of].ravel(),
                               prob.intr[self.zi, self.zk]])

    def pack(self, prob):
        return self._pack_full(prob)[self.keep]

    def unpack(self, x, prob):
        """Writes the free scalars only: a constant scalar keeps its bits."""
        prob.points[self.pt_of] = x[:3 * self.np].reshape(-1, 3)
        e = prob.ext[self.ext_of]
        e[self.ext_free] = x[3 * self.np:self.n_pc]
        prob.ext[self.ext_of] = e
        prob.intr[self.zi, self.zk] = x[self.n_pc:]

    def expand(self, M):
        """A square matrix over this layout's columns -> over the full layout's, zeros elsewhere."""
        F = np.zeros((self.n_full, self.n_full))
        F[np.ix_(self.keep, self.keep)] = M
        return F


def _append_rows(L, eff, J):
    """lm_ref.append_rows over a SubLayout: the free scalars' columns of every prior's A."""
    if not eff:
        return J
    P = np.zeros((6 * len(eff), L.n_full))
    for i, (c, A, _) in enumerate(eff):
        P[6 * i:6 * i + 6, 3 * L.np + 6 * c:3 * L.np + 6 * c + 6] = A
    return np.vstack([J, P[:, L.keep]])


@contextmanager
def _bound(bits):
    """lm_ref with SubLayout(bits) as its Layout and the prior rows over its columns."""
    saved = lr.Layout, lr.append_rows
    lr.Layout = lambda prob, const=None, groups=0: SubLayout(prob, const, groups, bits)
    lr.append_rows = _append_rows
    try:
        yield
    finally:
        lr.Layout, lr.append_rows = saved


def lm(pkg, orc, prob, opts, *, bits=None, **kw):
    """lm_ref.lm with the scalars of `bits` held constant (bit k of bits[e] = scalar k of ext[e])."""
    with _bound(bits):
        return lr.lm(pkg, orc, prob, opts, **kw)


def jacobian(pkg, orc, prob, *, bits=None, **kw):
    with _bound(bits):
        return lr.jacobian(pkg, orc, prob, **kw)


def covariance(pkg, orc, prob, *, bits=None, priors=None, const=None, groups=0, loss=lr.TRIVIAL):
    """lm_ref.covariance over the free scalars, with exact-zero rows and columns put back for the
    constant ones: the arrays of dab_covariance(_intrinsics), kappa and the rank test of the
    system without those columns, num_parameters over the free scalars."""
    L, A, cost = jacobian(pkg, orc, prob, bits=bits, priors=priors, const=const, groups=groups, loss=loss)
    out = czr.blocks(L.expand(cr.sigma_inv(A)), L, prob)
    out["point_cov"][L.const_of] = 0.0
    if L.nz == 0:
        out["ext_full"] = out["cam_full"]
    out.update(kappa=cr.kappa(A), cost=cost, num_parameters=L.n, num_residuals=A.shape[0], num_free_scalars=L.nz,
               layout=L, rank=czr.rank_test(A, L), ext_free=L.ext_free)
    return out


def rank(pkg, orc, prob, *, bits=None, **kw):
    """(rank test, kappa) alone: what the gauge table needs, also where Sigma does not exist."""
    L, A, _ = jacobian(pkg, orc, prob, bits=bits, **kw)
    return czr.rank_test(A, L), cr.kappa(A)


# ---- the shared cases and masks -------------------------------------------------------------------
def rot_odd(prob):
    e = np.arange(prob.ext.shape[0])
    return np.where(e % 2 == 1, ROTATION, 0).astype(np.uint8)


def trans_all(prob):
    return np.full(prob.ext.shape[0], TRANSLATION, np.uint8)


def mix(prob):
    e = np.arange(prob.ext.shape[0])
    return ((37 * e + 11) & 63).astype(np.uint8)


CASES = {"Blow": pr.case_b_low, "R": pr.case_r}
MASKS = {"rot-odd": rot_odd, "trans-all": trans_all, "mix": mix}
CAUCHY2 = (rr.CAUCHY, 2.0)
# (case, mask, loss, max_num_iterations)
TRAJECTORIES = [(c, m, None, 25) for c in ("Blow", "R") for m in ("rot-odd", "trans-all", "mix")] + [
    ("Blow", "mix", CAUCHY2, 15), ("R", "trans-all", CAUCHY2, 15)]
# the gauge table: (problem, extrinsic, bit of the translation scalar that fixes the scale)
GAUGE = {"bal40": (lambda pkg: cr.bal40(pkg, ()), 1, 3), "rig6x20": (lambda pkg: cr.rig6x20(pkg, ()), 1, 4)}


def one_bit(prob, e, k):
    b = np.zeros(prob.ext.shape[0], np.uint8)
    b[e] = 1 << k
    return b


def traj_id(t):
    return f"{t[0]}-{t[1]}" + ("-cauchy" if t[2] else "")
