"""TEST INFRASTRUCTURE ONLY: the reference for the extrinsic-prior tests (a plain module).

A prior on extrinsic e is Ceres' NormalPrior(A, mu) with a NULL loss on that block: the residual
block r = A (x_e - mu), x_e = ext[e] as stored. The reference is ptconst_ref's LM and covariance
over the same layout with the prior rows appended to the dense Jacobian:
  * A's 6 rows in the camera's 6 columns, after the observations' rows; A (x - mu) appended to the
    residual vector; 0.5 |A (x - mu)|^2 added to the evaluated and to the candidate cost;
  * priors on extrinsics outside L.ext_of (constant, unreferenced, freeze_camera) are skipped
    entirely, the library's documented simplification; num_residuals += 6 per effective prior;
  * lm(): ptconst_ref.lm statement by statement; with no priors it is ptconst_ref.lm bit for bit
    (tests/test_prior_ref.py pins that).
Also the prior sets and the cases the CPU and GPU tests share.
"""
import numpy as np

import cov_intr_ref as czr
import cov_ref as cr
import intr_ref as ir
import ptconst_ref as pr
import robust_ref as rr

DBL_MAX = rr.DBL_MAX


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


def lm(pkg, orc, prob, opts, priors=None, const=None, groups=0, loss=(rr.TRIVIAL, 1.0)):
    """ptconst_ref.lm with the prior rows, in place on prob.points / prob.ext / prob.intr. Returns a
    dict shaped like core.summary_to_dict."""
    kind, a = loss
    L = pr._Layout(prob, const, groups)
    eff = effective(L, priors)
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
        J21 = np.concatenate([J, ir.jz(p)], axis=2)
        rt, Jt, ps = rr.correct(kind, a, r, J21)
        A = L.dense(Jt[:, :, :15], Jt[:, :, 15:])
        rv = rt.ravel()
        cost = 0.5 * ps.sum()
        if eff:
            rp = prior_residuals(L, eff, p)
            A = append_rows(L, eff, A)
            rv = np.concatenate([rv, rp])
            cost = cost + 0.5 * (rp * rp).sum()
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
        out.update(num_iterations=0, termination="CONVERGENCE", message=pr.NO_FREE_MESSAGE, final_cost=x_cost,
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
        out["num_iterations"] = iteration
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


def cost_and_gradient(pkg, orc, prob, priors=None, const=None, groups=0, loss=(rr.TRIVIAL, 1.0)):
    """(layout, cost, gradient over the layout's columns) at prob's parameters."""
    L, J, cost = pr.jacobian(pkg, orc, prob, const, groups, loss)
    eff = effective(L, priors)
    r, J15 = orc.eval_jacobians(pkg, prob)
    J21 = np.concatenate([J15, ir.jz(prob)], axis=2)
    rt, _, _ = rr.correct(loss[0], loss[1], r, J21)
    rp = prior_residuals(L, eff, prob)
    rv = np.concatenate([rt.ravel(), rp])
    A = append_rows(L, eff, J)
    return L, cost + 0.5 * (rp * rp).sum(), A.T @ rv


def covariance(pkg, orc, prob, priors=None, const=None, groups=0, loss=(rr.TRIVIAL, 1.0)):
    """ptconst_ref.covariance with the prior rows appended to the Jacobian."""
    L, A, cost = pr.jacobian(pkg, orc, prob, const, groups, loss)
    eff = effective(L, priors)
    rp = prior_residuals(L, eff, prob)
    A = append_rows(L, eff, A)
    out = czr.blocks(cr.sigma_inv(A), L, prob)
    out["point_cov"][L.const_of] = 0.0
    out.update(kappa=cr.kappa(A), cost=cost + 0.5 * (rp * rp).sum(), num_parameters=L.n, num_residuals=A.shape[0],
               num_free_scalars=L.nz, num_effective=len(eff), layout=L,
               rank=cr.rank_test(A, type("N", (), dict(np=L.np, nc=L.nc + int(L.nz > 0)))()))
    return out


# ---- the shared prior sets ----------------------------------------------------------------------
SIG_W, SIG_T, SIG_POS = 0.02, 0.05, 0.01


def pose(prob, seed=11, groups=0):
    """A full prior on every free extrinsic, in L.ext_of's order: A = Q D (I + 0.2 G), Q from the QR
    of a normal draw, D = diag(1/0.02 x3, 1/0.05 x3), G a normal draw; mu = start + sigma o normal."""
    rng = np.random.default_rng(seed)
    L = pr._Layout(prob, None, groups)
    sig = np.array([SIG_W] * 3 + [SIG_T] * 3)
    idx, mu, A = [], [], []
    for e in L.ext_of:
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        G = rng.standard_normal((6, 6))
        A.append(Q @ np.diag(1.0 / sig) @ (np.eye(6) + 0.2 * G))
        mu.append(prob.ext[e] + sig * rng.standard_normal(6))
        idx.append(e)
    return np.array(idx, np.int32), np.array(mu).reshape(-1, 6), np.array(A).reshape(-1, 6, 6)


def pos3(prob, seed=11, which=None):
    """A position-only prior (zero rotation rows, I / 0.01 on the translation) on the first, the
    middle and the last free extrinsic (or on `which`); mu = the start translation + 0.01 o normal."""
    rng = np.random.default_rng(seed)
    L = pr._Layout(prob, None, 0)
    ext = L.ext_of if which is None else np.asarray(which)
    if which is None:
        ext = np.array([ext[0], ext[len(ext) // 2], ext[-1]])
    A1 = np.zeros((6, 6))
    A1[3:, 3:] = np.eye(3) / SIG_POS
    mu = prob.ext[ext].copy()
    mu[:, 3:] += SIG_POS * rng.standard_normal((len(ext), 3))
    return ext.astype(np.int32), mu, np.repeat(A1[None], len(ext), axis=0)


PRIORS = {"pose": pose, "pos3": pos3}


def shape_a7(pkg, orc):
    return ir.shape_a(pkg, orc)


# (name, case, prior set, constant mask, loss, free-intrinsic groups, max_num_iterations)
TRAJECTORIES = [
    ("B-pose", "B", "pose", None, None, 0, 25),
    ("B-pos3", "B", "pos3", None, None, 0, 25),
    ("B-pose-all", "B", "pose", "all", None, 0, 25),
    ("B-pose-third-cauchy", "B", "pose", "third", pr.CAUCHY2, 0, 15),
    ("R-pose", "R", "pose", None, None, 0, 25),
    ("R-pos3", "R", "pos3", None, None, 0, 25),
    ("R-pose-all", "R", "pose", "all", None, 0, 25),
    ("R2-pose-all", "R2", "pose", "all", None, 0, 25),
    ("Bragged-pose", "Bragged", "pose", None, None, 0, 25),
    ("A-pose-groups7", "A", "pose", None, None, 7, 25),
]
REJECTED = ("B-pose", "B-pos3", "R2-pose-all")  # trajectories with rejected steps


def traj_id(t):
    return t[0]


def make_case(pkg, orc, t):
    """(problem, priors, constant mask or None, loss, groups, iterations) of a trajectory."""
    _, case, pset, mask, loss, groups, iters = t
    prob = shape_a7(pkg, orc) if case == "A" else pr.CASES[case](pkg)
    m = pr.MASKS[mask](prob) if mask else None
    return prob, PRIORS[pset](prob), m, loss or (rr.TRIVIAL, 1.0), groups, iters
