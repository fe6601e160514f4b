"""TEST INFRASTRUCTURE ONLY: the reference for the robust-loss tests (a plain module).

oracle/ restates the reference's NULL-loss solve and cannot grow a loss, so the robust LM is
pinned here instead:
  * the loss table (Ceres' HuberLoss / SoftLOneLoss / CauchyLoss, restated in include/dab.h)
    and Ceres' Corrector in its first branch (rho'' <= 0 for all three: residual and Jacobian
    rows scaled by sqrt(rho'), alpha = 0), in numpy;
  * lm(): a dense trust-region LM over raw r, J from the oracle's orc_eval_jacobians. The
    normal equations over all free parameters are solved exactly, which is mathematically the
    Schur step; the loop follows oracle/dab_oracle.c (orc_solve) statement by statement.
With the TRIVIAL loss lm() must reproduce orc_solve (tests/test_robust_ref.py pins that);
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


class _Layout:
    """Free parameters of a problem, as orc_solve numbers them: referenced points (3 each) in
    id order, then referenced non-constant extrinsics (6 each) in id order."""

    def __init__(self, prob):
        npts, next_ = prob.points.shape[0], prob.ext.shape[0]
        pref = np.zeros(npts, bool)
        pref[prob.obs_point] = True
        eref = np.zeros(next_, bool)
        eref[prob.obs_ext0] = True
        eref[prob.obs_ext1[prob.obs_ext1 >= 0]] = True
        const = np.zeros(next_, bool) if prob.ext_const is None else prob.ext_const.astype(bool)
        if prob.freeze_camera:
            const[:] = True
        self.pt_of = np.flatnonzero(pref)
        self.ext_of = np.flatnonzero(eref & ~const)
        self.np, self.nc = len(self.pt_of), len(self.ext_of)
        self.n = 3 * self.np + 6 * self.nc
        pidx = -np.ones(npts, np.int64)
        pidx[self.pt_of] = np.arange(self.np)
        cidx = -np.ones(next_ + 1, np.int64)  # [-1] stays -1 (ext1 < 0)
        cidx[self.ext_of] = np.arange(self.nc)
        N = prob.num_obs
        col = -np.ones((N, 15), np.int64)
        col[:, 0:3] = 3 * pidx[prob.obs_point][:, None] + np.arange(3)
        for ext, k0 in ((prob.obs_ext0, 3), (prob.obs_ext1, 9)):
            ce = cidx[ext]
            ok = ce >= 0
            col[ok, k0:k0 + 6] = 3 * self.np + 6 * ce[ok][:, None] + np.arange(6)
        self.col = col

    def pack(self, prob):
        return np.concatenate([prob.points[self.pt_of].ravel(), prob.ext[self.ext_of].ravel()])

    def unpack(self, x, prob):
        prob.points[self.pt_of] = x[:3 * self.np].reshape(-1, 3)
        prob.ext[self.ext_of] = x[3 * self.np:].reshape(-1, 6)

    def dense(self, J):
        """[2 N][n] dense Jacobian from the [N][2][15] rows (constant blocks dropped)."""
        N = J.shape[0]
        A = np.zeros((2 * N, self.n))
        o, k = np.nonzero(self.col >= 0)
        c = self.col[o, k]
        A[2 * o, c] = J[o, 0, k]
        A[2 * o + 1, c] = J[o, 1, k]
        return A


def lm(pkg, orc, prob, opts, loss=(TRIVIAL, 1.0)):
    """Trust-region LM with an exact step under `loss` = (kind, scale), in place on
    prob.points / prob.ext. Returns a dict shaped like core.summary_to_dict."""
    kind, a = loss
    L = _Layout(prob)
    n = L.n
    work = prob.copy()  # evaluation point
    cand = prob.copy()
    x = L.pack(prob)
    x_norm = np.sqrt((x * x).sum())
    its = []
    state = {}

    def evaluate(p):
        r, J = orc.eval_jacobians(pkg, p)
        ok = bool(np.isfinite(r).all())
        rt, Jt, ps = correct(kind, a, r, J)
        A = L.dense(Jt)
        rv = rt.ravel()
        g = A.T @ rv
        state.update(A=A, r=rv, g=g)
        d = x - (x + (-g))
        return 0.5 * ps.sum(), (np.abs(d).max() if n else 0.0), ok

    iteration = 0
    radius, decrease_factor = opts.initial_trust_region_radius, 2.0
    minimum_cost = DBL_MAX
    xbest = x.copy()
    num_invalid = 0
    out = dict(num_successful_steps=0, num_unsuccessful_steps=0, num_parameters=n,
               num_free_points=L.np, num_free_ext=L.nc, num_residuals=2 * prob.num_obs)
    x_cost, gmax, ok = evaluate(work)
    scale = np.ones(n)
    if opts.jacobi_scaling:
        scale = 1.0 / (1.0 + np.sqrt((state["A"] ** 2).sum(axis=0)))
    out["initial_cost"] = x_cost
    final_cost_min = x_cost
    term, message = "FAILURE", ""
    if not ok:
        message = "Residual and Jacobian evaluation failed."
    step_is_successful, step_is_valid = True, True
    cost_change = step_norm = rel_decrease = 0.0
    iter_cost = x_cost
    while ok:
        if step_is_successful:
            out["num_successful_steps"] += 1
            if x_cost < minimum_cost:
                minimum_cost = x_cost
                xbest = x.copy()
        else:
            out["num_unsuccessful_steps"] += 1
        final_cost_min = min(final_cost_min, iter_cost)
        its.append(dict(iteration=iteration, success=bool(step_is_successful), valid=bool(step_is_valid),
                        cost=iter_cost, cost_change=cost_change, gradient_max_norm=gmax, step_norm=step_norm,
                        relative_decrease=rel_decrease, trust_region_radius=radius))
        out["num_iterations"] = iteration  # the index of the last record, as orc_solve
        if iteration >= opts.max_num_iterations:
            term = "NO_CONVERGENCE"
            message = f"Maximum number of iterations reached. Number of iterations: {iteration}."
            break
        if step_is_successful and gmax <= opts.gradient_tolerance:
            term, message = "CONVERGENCE", "Gradient tolerance reached."
            break
        if radius <= opts.min_trust_region_radius:
            term, message = "CONVERGENCE", "Minimum trust region radius reached."
            break
        iteration += 1
        prev_gmax = gmax
        step_is_successful = step_is_valid = False
        cost_change = step_norm = rel_decrease = 0.0

        A, r, g = state["A"], state["r"], state["g"]
        As = A * scale
        d = np.clip((As * As).sum(axis=0), opts.min_lm_diagonal, opts.max_lm_diagonal)
        Dd = np.sqrt(d / radius)
        H = As.T @ As + np.diag(Dd * Dd)
        solve_fail = False
        try:
            C = np.linalg.cholesky(H)
            y = np.linalg.solve(C.T, np.linalg.solve(C, g * scale))
            solve_fail = not np.isfinite(y).all()
        except np.linalg.LinAlgError:
            solve_fail = True
        model_cost_change = 0.0
        if not solve_fail:
            delta = -y * scale
            m = A @ delta
            model_cost_change = float((-(m * (r + m / 2.0))).sum())
            step_is_valid = model_cost_change > 0.0
        if not step_is_valid:
            num_invalid += 1
            if num_invalid >= opts.max_num_consecutive_invalid_steps:
                term = "FAILURE"
                message = "Number of consecutive invalid steps more than max_num_consecutive_invalid_steps"
                break
            radius /= decrease_factor
            decrease_factor *= 2.0
            iter_cost, cost_change, gmax = x_cost, 0.0, prev_gmax
            continue
        num_invalid = 0
        xc = x + delta
        L.unpack(xc, cand)
        rc, _ = orc.eval_residuals(pkg, cand)
        candidate_cost = cost(kind, a, rc) if np.isfinite(rc).all() else DBL_MAX
        step_norm = np.sqrt(((x - xc) ** 2).sum())
        if step_norm <= opts.parameter_tolerance * (x_norm + opts.parameter_tolerance):
            term, message = "CONVERGENCE", "Parameter tolerance reached."
            break
        cost_change = x_cost - candidate_cost
        if abs(cost_change) <= opts.function_tolerance * x_cost:
            term, message = "CONVERGENCE", "Function tolerance reached."
            break
        rel_decrease = (x_cost - candidate_cost) / model_cost_change
        if rel_decrease > opts.min_relative_decrease:
            x = xc
            L.unpack(x, work)
            x_norm = np.sqrt((x * x).sum())
            x_cost, gmax, ok = evaluate(work)
            if not ok:
                term, message = "FAILURE", "Residual and Jacobian evaluation failed."
                break
            step_is_successful = True
            iter_cost = x_cost
            radius = min(radius / max(1.0 / 3.0, 1.0 - (2.0 * rel_decrease - 1.0) ** 3),
                         opts.max_trust_region_radius)
            decrease_factor = 2.0
        else:
            step_is_successful = False
            iter_cost, gmax = candidate_cost, prev_gmax
            radius /= decrease_factor
            decrease_factor *= 2.0
    if minimum_cost < DBL_MAX:
        L.unpack(xbest, prob)
    out.setdefault("num_iterations", 0)
    out.update(termination=term, message=message, final_cost=final_cost_min, iterations=its)
    return out


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


def robust_triplet(pkg, orc, solve=None, iterations=25):
    """Inlier RMS on bal-small after a solve of (a) clean data, no loss; (b) contaminated
    data, no loss; (c) contaminated data, Cauchy(0.5). solve(problem, loss) runs in place;
    the default is lm()."""
    opts = pkg.options(max_num_iterations=iterations, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)
    if solve is None:
        def solve(p, loss):
            lm(pkg, orc, p, opts, loss)
    clean, _ = bal_small(pkg, orc, contaminated=False)
    dirty, out = bal_small(pkg, orc)
    res = []
    for prob, loss in ((clean, (TRIVIAL, 1.0)), (dirty.copy(), (TRIVIAL, 1.0)), (dirty.copy(), (CAUCHY, 0.5))):
        solve(prob, loss)
        res.append(inlier_rms(pkg, orc, prob, out))
    return tuple(res)
