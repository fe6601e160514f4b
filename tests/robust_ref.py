"""TEST INFRASTRUCTURE ONLY: the loss table and the cases of the robust-loss tests (a plain module).

oracle/ restates the reference's NULL-loss solve and cannot grow a loss, so the robust LM is
pinned by lm_ref.lm over what is here:
  * the loss table (Ceres' HuberLoss / SoftLOneLoss / CauchyLoss, restated in include/dab.h)
    and Ceres' Corrector in its first branch (rho'' <= 0 for all three: residual and Jacobian
    rows scaled by sqrt(rho'), alpha = 0), in numpy.
With the TRIVIAL loss lm_ref.lm must reproduce orc_solve (tests/test_robust_ref.py pins that);
parity of the robust path against Ceres itself stays unpinned, as for the oracle.
Also the small contaminated problems that the CPU and GPU tests share.
"""
import numpy as np

TRIVIAL, HUBER, SOFT_L1, CAUCHY = 0, 1, 2, 3
DBL_MIN = np.finfo(np.float64).tiny
DBL_MAX = np.finfo(np.float64).max


def rho(kind, a, s):
    """(rho(s), rho'(s)) of loss `kind` with scale a, elementwise."""
    s = np.asarray(s, np.float64)
    if kind == TRIVIAL:
        return s.copy(), np.ones_like(s)
    b = a * a
    c = 1.0 / b
    if kind == HUBER:
        r = np.sqrt(s)
        inside = s <= b
        with np.errstate(divide="ignore"):
            out = np.maximum(DBL_MIN, a / r)
        return np.where(inside, s, 2.0 * a * r - b), np.where(inside, 1.0, out)
    if kind == SOFT_L1:
        t = np.sqrt(1.0 + s * c)
        return 2.0 * b * (t - 1.0), np.maximum(DBL_MIN, 1.0 / t)
    if kind == CAUCHY:
        u = 1.0 + s * c
        return b * np.log(u), np.maximum(DBL_MIN, 1.0 / u)
    raise ValueError(kind)


def correct(kind, a, r, J):
    """Corrector, first branch: (sqrt(rho') r, sqrt(rho') J, rho(s)) per observation."""
    s = (r * r).sum(axis=1)
    p, p1 = rho(kind, a, s)
    w = np.sqrt(p1)
    return r * w[:, None], J * w[:, None, None], p


def cost(kind, a, r):
    return 0.5 * rho(kind, a, (r * r).sum(axis=1))[0].sum()


# ---- the small problems of the robust tests --------------------------------------------------
def _ragged(base, rng, lo, hi):
    """Keep the first k_p observations of every track, k_p uniform in [lo, hi] (track 0: 1)."""
    keep_n = rng.integers(lo, hi + 1, size=base.points.shape[0])
    keep_n[0] = 1
    order = np.argsort(base.obs_point, kind="stable")
    pts = base.obs_point[order]
    first = np.r_[0, np.flatnonzero(np.diff(pts)) + 1]
    start = np.repeat(first, np.diff(np.r_[first, len(pts)]))
    rank = np.zeros(base.num_obs, np.int64)
    rank[order] = np.arange(len(pts)) - start
    return base.subset(rank < keep_n[base.obs_point]).copy()


def contaminate(pkg, orc, prob, seed, frac=0.05):
    """5 % of the observations displaced by 30-60 px; among the others one set to its exact
    projection (s ~ 0) and one put within 1e-9 of Huber(1.0)'s switch s = b = 1. Returns the
    boolean mask of the displaced observations (the outliers)."""
    rng = np.random.default_rng(seed)
    N = prob.num_obs
    out = np.zeros(N, bool)
    out[rng.choice(N, size=max(1, int(round(frac * N))), replace=False)] = True
    ang = rng.uniform(0.0, 2.0 * np.pi, size=N)
    mag = rng.uniform(30.0, 60.0, size=N)
    prob.obs_xy[out] += (mag[:, None] * np.c_[np.cos(ang), np.sin(ang)])[out]
    r, _ = orc.eval_residuals(pkg, prob)
    i0, i1 = np.flatnonzero(~out)[[3, 11]]
    prob.obs_xy[i0] += r[i0]                      # residual 0
    u = np.array([0.6, 0.8]) * np.sqrt(1.0 + 5e-10)
    prob.obs_xy[i1] += r[i1] - u                  # residual u, |u|^2 = 1 + 5e-10
    return out


def bal_small(pkg, orc, seed=5, contaminated=True):
    """BAL-shaped: 12 cameras, 200 points (4 SELL slices, the last partial), ragged tracks of
    1-8 observations (padding slots, single-observation points)."""
    base = pkg.synth(kind=0, num_cameras=12, num_points=200, obs_per_point=8, seed=seed)
    prob = _ragged(base, np.random.default_rng(seed), 1, 8)
    mask = contaminate(pkg, orc, prob, seed) if contaminated else np.zeros(prob.num_obs, bool)
    return prob, mask


def rig_small(pkg, orc, seed=6, contaminated=True):
    """Rig: 3 arcs x 5 rings, 200 points, 6 observations per point."""
    prob = pkg.synth(kind=1, num_arcs=3, num_rings=5, num_points=200, obs_per_point=6, seed=seed)
    mask = contaminate(pkg, orc, prob, seed) if contaminated else np.zeros(prob.num_obs, bool)
    return prob, mask


def scaled_blocks(prob, r, J, loss):
    """Host sums of the sqrt(rho')-scaled rows, in dab_bench_get_blocks' layout: V [points][6],
    g [points][3], ug [free ext][27], the sum of the cross blocks, and 0.5 sum rho."""
    rt, Jt, ps = correct(loss[0], loss[1], r, J)
    iu3, iu6 = np.triu_indices(3), np.triu_indices(6)
    npts, next_ = prob.points.shape[0], prob.ext.shape[0]
    Jp = Jt[:, :, :3]
    V = np.zeros((npts, 3, 3))
    g = np.zeros((npts, 3))
    np.add.at(V, prob.obs_point, np.einsum("oki,okj->oij", Jp, Jp))
    np.add.at(g, prob.obs_point, np.einsum("oki,ok->oi", Jp, rt))
    U = np.zeros((next_, 6, 6))
    gc = np.zeros((next_, 6))
    ref = np.zeros(next_, bool)
    for ext, cols in ((prob.obs_ext0, slice(3, 9)), (prob.obs_ext1, slice(9, 15))):
        m = ext >= 0
        Jc = Jt[m][:, :, cols]
        np.add.at(U, ext[m], np.einsum("oki,okj->oij", Jc, Jc))
        np.add.at(gc, ext[m], np.einsum("oki,ok->oi", Jc, rt[m]))
        ref[ext[m]] = True
    const = np.zeros(next_, bool) if prob.ext_const is None else prob.ext_const.astype(bool)
    free = np.flatnonzero(ref & ~const)
    both = (prob.obs_ext1 >= 0) & ~const[prob.obs_ext0] & ~const[np.maximum(prob.obs_ext1, 0)]
    cross = np.einsum("oki,okj->", Jt[both][:, :, 3:9], Jt[both][:, :, 9:15])
    ug = np.concatenate([U[free][:, iu6[0], iu6[1]], gc[free]], axis=1)
    return dict(V=V[:, iu3[0], iu3[1]], g=g, ug=ug, cross=cross, cost=0.5 * ps.sum())


def inlier_rms(pkg, orc, prob, outliers):
    """RMS of |r| over the observations that were not displaced, at prob's parameters."""
    r, _ = orc.eval_residuals(pkg, prob)
    return float(np.sqrt((r[~outliers] ** 2).sum(axis=1).mean()))

