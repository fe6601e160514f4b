"""TEST INFRASTRUCTURE ONLY: the one reference trust-region loop of the GPU tests (a plain module).

oracle/ restates the reference's solve with a NULL loss, constant intrinsics, free points and no
priors, and cannot grow any of the four. Every feature test is judged against this module instead:
  * Layout: the free parameters as Ceres' reduced program has them: referenced non-constant points
    (3 each) in id order, referenced non-constant extrinsics (6 each) in id order, then the active
    scalars of the free intrinsics in (index, slot) order;
  * corrected_rows / linearize: the one linearisation. The oracle's rows beside intr_ref.jz's six
    intrinsic columns, scaled by sqrt(rho') (robust_ref.correct), made dense over the layout, with
    the rows A and residuals A (x_e - mu) of the priors on free extrinsics under the observations';
  * lm(): a dense trust-region LM over that. The normal equations over all free parameters are
    solved exactly, which is mathematically the Schur step; the loop follows oracle/dab_oracle.c
    (orc_solve) statement by statement. No free parameter at all gives Ceres' "No non-constant
    parameter blocks found" summary;
  * jacobian / cost_and_gradient / covariance: the same linearisation at one point; covariance
    returns the arrays of dab_covariance and dab_covariance_intrinsics (cov_intr_ref.blocks), rows
    of constant points exactly 0 (known exactly), unreferenced points NaN.
Priors on extrinsics outside Layout.ext_of (constant, unreferenced, freeze_camera) are skipped
entirely, the library's documented simplification; num_residuals += 6 per effective prior.

What pins lm(): the oracle at the TRIVIAL loss with groups = 0 (tests/test_robust_ref.py,
tests/test_intr_ref.py), and everywhere else the outputs of the four loops it replaced, recorded
in tests/golden/lm_ref_parent.json (oracle/gen_lm_ref_golden.py, tests/test_lm_ref.py). Parity of
the features against Ceres itself stays unpinned, as for the oracle. The loss table, jz and the
cases, masks and prior sets live in robust_ref, intr_ref, ptconst_ref and prior_ref.
"""
import numpy as np

import cov_intr_ref as czr
import cov_ref as cr
import intr_ref as ir
import robust_ref as rr

DBL_MAX = rr.DBL_MAX
TRIVIAL = (rr.TRIVIAL, 1.0)
NO_FREE_MESSAGE = "Function tolerance reached. No non-constant parameter blocks found."


def as_mask(prob, const):
    """[num_points] bool from None / a bool / an array (any non-zero entry = constant)."""
    npts = prob.points.shape[0]
    if const is None:
        return np.zeros(npts, bool)
    m = np.asarray(const)
    if m.ndim == 0:
        return np.full(npts, bool(m))
    assert m.shape == (npts,)
    return m != 0


class Layout:
    """The free parameters of a problem (module docstring). const_of: the referenced constant
    points (unreferenced flagged points are ignored, as unreferenced blocks are). col [N][15] and
    zcol [N][6]: the column of every entry of an observation's rows, -1 where it has none."""

    def __init__(self, prob, const=None, groups=0):
        npts, next_ = prob.points.shape[0], prob.ext.shape[0]
        pref = np.zeros(npts, bool)
        pref[prob.obs_point] = True
        eref = np.zeros(next_, bool)
        eref[prob.obs_ext0] = True
        eref[prob.obs_ext1[prob.obs_ext1 >= 0]] = True
        econst = np.zeros(next_, bool) if prob.ext_const is None else prob.ext_const.astype(bool)
        if prob.freeze_camera:
            econst[:] = True
        cm = as_mask(prob, const)
        self.pt_of = np.flatnonzero(pref & ~cm)
        self.const_of = np.flatnonzero(pref & cm)
        self.ext_of = np.flatnonzero(eref & ~econst)
        self.act = ir.active_mask(prob, groups)
        self.zi, self.zk = np.nonzero(self.act)
        self.np, self.nc, self.nz = len(self.pt_of), len(self.ext_of), len(self.zi)
        self.n_pc = 3 * self.np + 6 * self.nc
        self.n = self.n_pc + self.nz
        pidx = -np.ones(npts, np.int64)
        pidx[self.pt_of] = np.arange(self.np)
        cidx = -np.ones(next_ + 1, np.int64)  # [-1] stays -1 (ext1 < 0)
        cidx[self.ext_of] = np.arange(self.nc)
        col = -np.ones((prob.num_obs, 15), np.int64)
        for idx, k0, w, base in ((pidx[prob.obs_point], 0, 3, 0), (cidx[prob.obs_ext0], 3, 6, 3 * self.np),
                                 (cidx[prob.obs_ext1], 9, 6, 3 * self.np)):
            ok = idx >= 0
            col[ok, k0:k0 + w] = base + w * idx[ok][:, None] + np.arange(w)
        self.col = col
        zcol = -np.ones(self.act.shape, np.int64)
        zcol[self.zi, self.zk] = self.n_pc + np.arange(self.nz)
        self.zcol = zcol[prob.obs_intr]

    def pack(self, prob):
        return np.concatenate([prob.points[self.pt_of].ravel(), prob.ext[self.ext_of].ravel(),
                               prob.intr[self.zi, self.zk]])

    def unpack(self, x, prob):
        prob.points[self.pt_of] = x[:3 * self.np].reshape(-1, 3)
        prob.ext[self.ext_of] = x[3 * self.np:self.n_pc].reshape(-1, 6)
        prob.intr[self.zi, self.zk] = x[self.n_pc:]

    def dense(self, J21):
        """[2 N][n] dense Jacobian from the [N][2][21] rows (blocks without a column dropped)."""
        col = np.concatenate([self.col, self.zcol], axis=1)
        A = np.zeros((2 * J21.shape[0], self.n))
        o, k = np.nonzero(col >= 0)
        c = col[o, k]
        A[2 * o, c] = J21[o, 0, k]
        A[2 * o + 1, c] = J21[o, 1, k]
        return A


# ---- the prior rows ---------------------------------------------------------------------------
def effective(L, priors):
    """[(camera column index in L.ext_of, A, mu)] of the priors whose extrinsic is free, in the
    order set. priors: None or (index [n], mean [n][6], sqrt_info [n][6][6])."""
    if priors is None:
        return []
    idx, mu, A = priors
    pos = {int(e): c for c, e in enumerate(L.ext_of)}
    return [(pos[int(e)], np.asarray(A[i], float), np.asarray(mu[i], float))
            for i, e in enumerate(idx) if int(e) in pos]


def prior_residuals(L, eff, prob):
    """[6 len(eff)] stacked A (x_e - mu)."""
    return np.concatenate([A @ (prob.ext[L.ext_of[c]] - mu) for c, A, mu in eff]) if eff else np.zeros(0)


def append_rows(L, eff, J):
    """The dense Jacobian with the priors' rows under the observations'."""
    if not eff:
        return J
    P = np.zeros((6 * len(eff), J.shape[1]))
    for i, (c, A, _) in enumerate(eff):
        P[6 * i:6 * i + 6, 3 * L.np + 6 * c:3 * L.np + 6 * c + 6] = A
    return np.vstack([J, P])


# ---- the linearisation ------------------------------------------------------------------------
def corrected_rows(pkg, orc, prob, loss):
    """(sqrt(rho') r [N][2], sqrt(rho') J [N][2][21], rho [N], r finite) at prob's parameters: the
    oracle's 15 columns, then jz's 6."""
    r, J = orc.eval_jacobians(pkg, prob)
    ok = bool(np.isfinite(r).all())
    rt, Jt, ps = rr.correct(loss[0], loss[1], r, np.concatenate([J, ir.jz(prob)], axis=2))
    return rt, Jt, ps, ok


def linearize(pkg, orc, prob, L, loss, eff):
    """(A, r, cost, ok): the dense Jacobian and the residual vector over L's columns, observations
    then effective priors; cost = 0.5 sum rho (+ 0.5 |prior residuals|^2)."""
    rt, Jt, ps, ok = corrected_rows(pkg, orc, prob, loss)
    A = L.dense(Jt)
    rv = rt.ravel()
    cost = 0.5 * ps.sum()
    if eff:
        rp = prior_residuals(L, eff, prob)
        A = append_rows(L, eff, A)
        rv = np.concatenate([rv, rp])
        cost = cost + 0.5 * (rp * rp).sum()
    return A, rv, cost, ok


def lm(pkg, orc, prob, opts, *, priors=None, const=None, groups=0, loss=TRIVIAL):
    """Trust-region LM with an exact step under `loss` = (kind, scale), with the points of `const`
    held constant, the active intrinsic scalars of `groups` as unknowns and `priors` on the
    extrinsics, in place on prob.points / prob.ext / prob.intr. Returns a dict shaped like
    core.summary_to_dict."""
    kind, a = loss
    L = Layout(prob, const, groups)
    eff = effective(L, priors)
    n = L.n
    work = prob.copy()  # evaluation point
    cand = prob.copy()
    x = L.pack(prob)
    x_norm = np.sqrt((x * x).sum())
    its = []
    state = {}

    def evaluate(p):
        A, rv, cost, ok = linearize(pkg, orc, p, L, loss, eff)
        g = A.T @ rv
        state.update(A=A, r=rv, g=g)
        d = x - (x + (-g))
        return cost, (np.abs(d).max() if n else 0.0), ok

    iteration = 0
    radius, decrease_factor = opts.initial_trust_region_radius, 2.0
    minimum_cost = DBL_MAX
    xbest = x.copy()
    num_invalid = 0
    out = dict(num_successful_steps=0, num_unsuccessful_steps=0, num_parameters=n,
               num_free_points=L.np, num_free_ext=L.nc, num_residuals=2 * prob.num_obs + 6 * len(eff))
    x_cost, gmax, ok = evaluate(work)
    out["initial_cost"] = x_cost
    if ok and n == 0:
        # Ceres' reduced program is empty: TrustRegionMinimizer never runs
        out.update(num_iterations=0, termination="CONVERGENCE", message=NO_FREE_MESSAGE, final_cost=x_cost,
                   iterations=[])
        return out
    scale = np.ones(n)
    if opts.jacobi_scaling:
        scale = 1.0 / (1.0 + np.sqrt((state["A"] ** 2).sum(axis=0)))
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
        candidate_cost = rr.cost(kind, a, rc) if np.isfinite(rc).all() else DBL_MAX
        if eff and candidate_cost < DBL_MAX:
            rp = prior_residuals(L, eff, cand)
            candidate_cost = candidate_cost + 0.5 * (rp * rp).sum() if np.isfinite(rp).all() else DBL_MAX
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


# ---- one point: Jacobian, gradient, covariance ------------------------------------------------
def jacobian(pkg, orc, prob, *, priors=None, const=None, groups=0, loss=TRIVIAL):
    """(layout, dense Jacobian of the loss-corrected rows with the prior rows under them, cost)."""
    L = Layout(prob, const, groups)
    A, _, cost, _ = linearize(pkg, orc, prob, L, loss, effective(L, priors))
    return L, A, cost


def cost_and_gradient(pkg, orc, prob, *, priors=None, const=None, groups=0, loss=TRIVIAL):
    """(layout, cost, gradient over the layout's columns) at prob's parameters."""
    L = Layout(prob, const, groups)
    A, rv, cost, _ = linearize(pkg, orc, prob, L, loss, effective(L, priors))
    return L, cost, A.T @ rv


def covariance(pkg, orc, prob, *, priors=None, const=None, groups=0, loss=TRIVIAL):
    """Everything a GPU test compares against, computed once per case: the arrays of
    dab_covariance_intrinsics from cov_ref.sigma_inv of the Jacobian (without a free scalar
    intr_cov is empty and cam_full is dab_covariance's ext_full, returned under that name too),
    point_cov rows of the referenced constant points exactly 0, kappa, the rank test, the cost and
    the sizes."""
    L = Layout(prob, const, groups)
    eff = effective(L, priors)
    A, _, cost, _ = linearize(pkg, orc, prob, L, loss, eff)
    out = czr.blocks(cr.sigma_inv(A), L, prob)
    out["point_cov"][L.const_of] = 0.0
    if L.nz == 0:
        out["ext_full"] = out["cam_full"]
    out.update(kappa=cr.kappa(A), cost=cost, num_parameters=L.n, num_residuals=A.shape[0], num_free_scalars=L.nz,
               num_effective=len(eff), layout=L, rank=czr.rank_test(A, L))
    return out


# ---- it is robust -------------------------------------------------------------------------------
def robust_triplet(pkg, orc, solve=None, iterations=25):
    """Inlier RMS on bal-small after a solve of (a) clean data, no loss; (b) contaminated
    data, no loss; (c) contaminated data, Cauchy(0.5). solve(problem, loss) runs in place;
    the default is lm()."""
    opts = pkg.options(max_num_iterations=iterations, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)
    if solve is None:
        def solve(p, loss):
            lm(pkg, orc, p, opts, loss=loss)
    clean, _ = rr.bal_small(pkg, orc, contaminated=False)
    dirty, out = rr.bal_small(pkg, orc)
    res = []
    for prob, loss in ((clean, TRIVIAL), (dirty.copy(), TRIVIAL), (dirty.copy(), (rr.CAUCHY, 0.5))):
        solve(prob, loss)
        res.append(rr.inlier_rms(pkg, orc, prob, out))
    return tuple(res)
