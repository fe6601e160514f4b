"""TEST INFRASTRUCTURE ONLY: the intrinsic columns and the shapes of the free-intrinsics tests (a
plain module).

oracle/ restates the reference's solve with constant intrinsics (sfm.cc:60-62) and cannot grow
intrinsic columns, so the self-calibrating LM is pinned by lm_ref.lm over what is here:
  * jz(): the six analytic columns d r / d (cx, cy, f0, f1, k0, k1) of every observation in
    numpy, for every (nf, nk), single and composed observations (checked against central
    differences of the oracle's residual in tests/test_intr_ref.py);
  * active_mask(): the scalars that lm_ref.Layout puts after the extrinsics.
lm_ref.lm's own summation order shows on one shape: with per-camera intrinsics and all groups
free the problem is weakly constrained, a one-ulp difference in an early step grows about 2.5
times per iteration, and over 15 iterations two listings of the same problem differ by
0.9e-10 .. 1.7e-10 of the cost (five orders tried; 4e-13 or less on the other shapes). That
is the float64 uncertainty of any implementation on that shape, the code under test included.
Also the shapes the CPU and GPU tests share.
"""
import numpy as np

import robust_ref as rr

CENTER, FOCAL, DISTORTION = 1, 2, 4


def _rot(w):
    """Rodrigues: [n][3] angle-axis -> [n][3][3]."""
    th = np.sqrt((w * w).sum(axis=1))
    K = np.zeros((w.shape[0], 3, 3))
    K[:, 0, 1], K[:, 0, 2] = -w[:, 2], w[:, 1]
    K[:, 1, 0], K[:, 1, 2] = w[:, 2], -w[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -w[:, 1], w[:, 0]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6.0, np.sin(ths) / ths)
    b = np.where(small, 0.5 - th * th / 24.0, (1.0 - np.cos(ths)) / (ths * ths))
    return np.eye(3)[None] + a[:, None, None] * K + b[:, None, None] * (K @ K)


def camera_points(prob):
    """P of every observation: R(w0) X + t0, or R(w0) (R(w1) X + t1) + t0 when composed."""
    X = prob.points[prob.obs_point]
    comp = prob.obs_ext1 >= 0
    e1 = prob.ext[np.maximum(prob.obs_ext1, 0)]
    Q = np.where(comp[:, None], np.einsum("nij,nj->ni", _rot(e1[:, :3]), X) + e1[:, 3:], X)
    e0 = prob.ext[prob.obs_ext0]
    return np.einsum("nij,nj->ni", _rot(e0[:, :3]), Q) + e0[:, 3:]


def struct_mask(prob):
    """[num_intr][6] bool: the scalars the model of each intrinsic has."""
    nf, nk = prob.intr_nf, prob.intr_nk
    m = np.zeros((prob.intr.shape[0], 6), bool)
    m[:, :3] = True
    m[:, 3] = nf == 2
    m[:, 4] = nk >= 1
    m[:, 5] = nk >= 2
    return m


def active_mask(prob, groups):
    """[num_intr][6] bool: scalars selected by the DAB_INTR_* groups (an int or one per intrinsic)
    of referenced intrinsics."""
    ni = prob.intr.shape[0]
    g = np.broadcast_to(np.asarray(groups, np.int64), (ni,))
    sel = np.zeros((ni, 6), bool)
    sel[:, 0:2] = (g & CENTER)[:, None] != 0
    sel[:, 2:4] = (g & FOCAL)[:, None] != 0
    sel[:, 4:6] = (g & DISTORTION)[:, None] != 0
    ref = np.zeros(ni, bool)
    ref[prob.obs_intr] = True
    return sel & struct_mask(prob) & ref[:, None] & (not prob.freeze_camera)


def jz(prob):
    """[N][2][6] raw d r / d (cx, cy, f0, f1, k0, k1); columns of scalars the model lacks are zero,
    with nf == 1 the f0 column carries both rows."""
    P = camera_points(prob)
    K = prob.intr[prob.obs_intr]
    nf = prob.intr_nf[prob.obs_intr]
    nk = prob.intr_nk[prob.obs_intr]
    xp, yp = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2]
    r2 = xp * xp + yp * yp
    k0 = np.where(nk >= 1, K[:, 4], 0.0)
    k1 = np.where(nk >= 2, K[:, 5], 0.0)
    d = 1.0 + r2 * (k0 + k1 * r2)
    fx = K[:, 2]
    fy = np.where(nf == 2, K[:, 3], K[:, 2])
    J = np.zeros((prob.num_obs, 2, 6))
    J[:, 0, 0] = 1.0
    J[:, 1, 1] = 1.0
    J[:, 0, 2] = d * xp
    J[:, 1, 2] = np.where(nf == 1, d * yp, 0.0)
    J[:, 1, 3] = np.where(nf == 2, d * yp, 0.0)
    J[:, 0, 4] = fx * r2 * xp
    J[:, 1, 4] = fy * r2 * yp
    J[:, 0, 5] = fx * r2 * r2 * xp
    J[:, 1, 5] = fy * r2 * r2 * yp
    return J * struct_mask(prob)[prob.obs_intr][:, None, :]


def scaled_intrinsic_blocks(prob, r, Jz, groups, loss):
    """Host sums of the sqrt(rho')-scaled intrinsic rows over the active columns, per free
    intrinsic in ascending index: [nfi][27] = U_zz upper 21 | g_z 6 (dab_get_intrinsic_blocks)."""
    rt, Jt, _ = rr.correct(loss[0], loss[1], r, Jz)
    act = active_mask(prob, groups)
    Jt = Jt * act[prob.obs_intr][:, None, :]
    ni = prob.intr.shape[0]
    U = np.zeros((ni, 6, 6))
    g = np.zeros((ni, 6))
    np.add.at(U, prob.obs_intr, np.einsum("oki,okj->oij", Jt, Jt))
    np.add.at(g, prob.obs_intr, np.einsum("oki,ok->oi", Jt, rt))
    free = np.flatnonzero(act.any(axis=1))
    iu = np.triu_indices(6)
    return np.concatenate([U[free][:, iu[0], iu[1]], g[free]], axis=1)


# ---- the shapes of the free-intrinsics tests -------------------------------------------------
def offset_intrinsics(prob):
    """The miscalibration of the tests: focal x 1.01, centre by (+3, -2) px, k0 by +0.01."""
    prob.intr[:, 2:4] *= 1.01
    prob.intr[:, 0] += 3.0
    prob.intr[:, 1] -= 2.0
    prob.intr[:, 4] += 0.01
    return prob


def shape_a(pkg, orc, contaminated=False):
    """rig_small with intr_nf = [1, 2, 1], intr_nk = [2, 1, 0]: composed observations, three
    shared intrinsics, inactive slots."""
    prob, _ = rr.rig_small(pkg, orc, contaminated=contaminated)
    assert prob.intr.shape[0] == 3
    prob.intr_nf[:] = [1, 2, 1]
    prob.intr_nk[:] = [2, 1, 0]
    return offset_intrinsics(prob)


def shape_b(pkg, orc, contaminated=False):
    """bal_small: twelve per-camera intrinsics, nf 1, nk 2, padding slots, single-observation
    points, rejected steps."""
    prob, _ = rr.bal_small(pkg, orc, contaminated=contaminated)
    return offset_intrinsics(prob)


def shape_c(pkg, orc):
    """bal_small with one intrinsic seen by every camera; pixels re-synthesised as the oracle's
    projection at the unperturbed parameters plus seeded N(0, 1) px noise."""
    prob, _ = rr.bal_small(pkg, orc, contaminated=False)
    prob.obs_intr[:] = 0
    r, _ = orc.eval_residuals(pkg, prob)
    rng = np.random.default_rng(17)
    prob.obs_xy[...] = prob.obs_xy + r + rng.normal(0.0, 1.0, size=prob.obs_xy.shape)
    return offset_intrinsics(prob)


def reorder(prob):
    """The same problem with its observations in another order (reversed)."""
    return prob.subset(np.arange(prob.num_obs)[::-1]).copy()
