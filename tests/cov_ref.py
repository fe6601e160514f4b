"""TEST INFRASTRUCTURE ONLY: the covariance mathematics of the numpy reference of dab_covariance
(a plain module).

Sigma = (J^T J)^-1 over the free parameters (lm_ref.Layout), J the dense Jacobian of
lm_ref.jacobian; lm_ref.covariance splits it into the call's arrays. Two routes, pinned against
each other by tests/test_cov_ref.py:
  * sigma_inv: inv of the Jacobi-scaled H = (J s)^T (J s), unscaled (the library's variables);
  * sigma_pinv: pinv(J) pinv(J)^T (the SVD route, what Ceres' DENSE_SVD computes).
Also kappa of the scaled H (the accuracy bound of the GPU tests is 64 kappa 2^-53 max|Sigma|),
the library's rank test (pivot ratios of unpivoted Cholesky factors of the scaled point blocks
and of the scaled Schur complement), and the problems the CPU and GPU tests share.
"""
import numpy as np

import robust_ref as rr

MIN_PIVOT_RATIO = 1e-10
EPS = 2.0 ** -53


def jacobi_scale(A, on=True):
    return 1.0 / (1.0 + np.sqrt((A * A).sum(axis=0))) if on else np.ones(A.shape[1])


def scaled_h(A, on=True):
    s = jacobi_scale(A, on)
    As = A * s
    return s, As.T @ As


def kappa(A):
    """2-norm condition number of the Jacobi-scaled H."""
    return float(np.linalg.cond(scaled_h(A)[1]))


def sigma_inv(A):
    s, H = scaled_h(A)
    return s[:, None] * np.linalg.inv(H) * s[None, :]


def sigma_pinv(A):
    P = np.linalg.pinv(A)
    return P @ P.T


def _chol_pivots(M):
    """Pivots d_j = m_jj - sum_k l_jk^2 of the unpivoted Cholesky of M, stopped at the first
    pivot that is not positive (returned last)."""
    n = M.shape[0]
    Lf = np.zeros_like(M)
    piv = []
    for j in range(n):
        d = M[j, j] - Lf[j, :j] @ Lf[j, :j]
        piv.append(d)
        if not d > 0.0:
            break
        Lf[j, j] = np.sqrt(d)
        Lf[j + 1:, j] = (M[j + 1:, j] - Lf[j + 1:, :j] @ Lf[j, :j]) / Lf[j, j]
    return np.array(piv)


def rank_test(A, L, thr=MIN_PIVOT_RATIO):
    """The library's rank test on the Jacobi-scaled H. Returns a dict: point_ratio [np] (min / max
    pivot of each point's 3x3 Cholesky), deficient_points (free-point indices whose ratio is not
    > thr), camera_ratio (min / max squared diagonal of the Cholesky factor of the scaled Schur
    complement; 0 when a pivot is not positive, None when a point already failed or there is no
    free camera), deficient (bool)."""
    _, H = scaled_h(A)
    n3 = 3 * L.np
    ratio = np.zeros(L.np)
    for p in range(L.np):
        piv = _chol_pivots(H[3 * p:3 * p + 3, 3 * p:3 * p + 3])
        # a factorisation that stopped early did so at a non-positive pivot: the minimum
        ratio[p] = piv.min() / piv.max() if piv[0] > 0.0 else -np.inf
    bad = np.flatnonzero(~(ratio > thr))
    out = dict(point_ratio=ratio, deficient_points=bad, camera_ratio=None, deficient=len(bad) > 0)
    if len(bad) or L.nc == 0:
        return out
    V, W, U = H[:n3, :n3], H[n3:, :n3], H[n3:, n3:]
    Vinv = np.zeros_like(V)
    for p in range(L.np):
        k = slice(3 * p, 3 * p + 3)
        Vinv[k, k] = np.linalg.inv(V[k, k])
    S = U - W @ Vinv @ W.T
    piv = _chol_pivots(0.5 * (S + S.T))
    cr = 0.0 if (len(piv) < S.shape[0] or not piv[-1] > 0.0) else float(piv.min() / piv.max())
    out.update(camera_ratio=cr, deficient=not cr > thr)
    return out


# ---- the shared problems ------------------------------------------------------------------
def _with_const(prob, extra):
    prob.ext_const[list(extra)] = 1
    return prob


def bal40(pkg, extra_const=(1,)):
    """BAL-shaped, 40 cameras, 200 points x 8; camera 0 constant (the synthesiser's gauge rule)
    plus extra_const. (1,): full rank, n = 228 (4 blocks of 64, the last 36 wide); (): gauge-free."""
    return _with_const(pkg.synth(kind=0, num_cameras=40, num_points=200, obs_per_point=8, seed=5), extra_const)


def bal170(pkg):
    """170 cameras (168 free > 160: pair tables by selection), 400 points x 8; n = 1008."""
    return _with_const(pkg.synth(kind=0, num_cameras=170, num_points=400, obs_per_point=8, seed=5), (1,))


def bal40_ragged(pkg):
    """bal40's base with tracks of 2-8 observations (padding slots); point 0 keeps one observation
    in robust_ref._ragged, which is removed here: an unreferenced point (NaN row)."""
    base = pkg.synth(kind=0, num_cameras=40, num_points=200, obs_per_point=8, seed=5)
    prob = rr._ragged(base, np.random.default_rng(5), 2, 8)
    prob = prob.subset(prob.obs_point != 0).copy()
    return _with_const(prob, (1,))


def rig(pkg, arcs, rings, obs, extra_const):
    """The rig as synthesised (arc 0 constant: the reference's gauge rule, scale free) plus
    extra_const."""
    return _with_const(pkg.synth(kind=1, num_arcs=arcs, num_rings=rings, num_points=200, obs_per_point=obs,
                                 seed=6), extra_const)


def rig3x5(pkg, extra_const=(3,)):
    return rig(pkg, 3, 5, 6, extra_const)   # n = 30 with (3,)


def rig6x20(pkg, extra_const=(1,)):
    return rig(pkg, 6, 20, 8, extra_const)  # n = 138 with (1,)


def freeze(pkg):
    prob = pkg.synth(kind=0, num_cameras=12, num_points=200, obs_per_point=8, seed=5)
    prob.freeze_camera = True
    return prob


WELL_POSED = {"bal40": bal40, "bal170": bal170, "bal40-ragged": bal40_ragged, "rig3x5": rig3x5,
              "rig6x20": rig6x20, "freeze": freeze}
DEFICIENT = {"bal40-gauge": lambda pkg: bal40(pkg, ()), "rig3x5-gauge": lambda pkg: rig3x5(pkg, ())}
