"""TEST INFRASTRUCTURE ONLY: the reference, prior sets and cases of the point-prior tests (a plain module).

A prior on point p is Ceres' NormalPrior(A, mu) with a NULL loss on that block: the residual block
r = A (X_p - mu), X_p = points[p], A 3x3. lm / jacobian / cost_and_gradient / covariance here take
`point_priors` = (index [n], mean [n][3], sqrt_info [n][3][3]) beside lm_ref's arguments and put the
3-row point blocks under the extrinsic priors' rows; everything else (Layout, corrected_rows,
effective, append_rows, prior_residuals) is lm_ref's. A prior on a point outside Layout.pt_of
(constant or unreferenced) is skipped entirely, the library's documented simplification;
num_residuals += 3 per effective prior.

lm() is a SECOND COPY of lm_ref.lm, statement for statement, with the point rows added: lm_ref.py
is a frozen test file for the change that added point priors and could not grow the argument.
tests/test_ptprior_ref.py pins the copy: with point_priors=None it returns lm_ref.lm's dict bit for
bit. The follow-up is to fold `point_priors` into lm_ref.lm / linearize and delete the copy.
"""
import numpy as np

import cov_intr_ref as czr
import cov_ref as cr
import intr_ref as ir
import lm_ref as lr
import prior_ref as qr
import ptconst_ref as pr
import robust_ref as rr

DBL_MAX = lr.DBL_MAX
TRIVIAL = lr.TRIVIAL


# ---- the point-prior rows ----------------------------------------------------------------------
def pt_effective(L, point_priors):
    """[(free point index in L.pt_of, A, mu)] of the priors whose point is free, in the order set."""
    if point_priors is None:
        return []
    idx, mu, A = point_priors
    pos = {int(p): c for c, p in enumerate(L.pt_of)}
    return [(pos[int(p)], np.asarray(A[i], float), np.asarray(mu[i], float))
            for i, p in enumerate(idx) if int(p) in pos]


def pt_prior_residuals(L, peff, prob):
    """[3 len(peff)] stacked A (X_p - mu)."""
    return np.concatenate([A @ (prob.points[L.pt_of[c]] - mu) for c, A, mu in peff]) if peff else np.zeros(0)


def pt_append_rows(L, peff, J):
    if not peff:
        return J
    P = np.zeros((3 * len(peff), J.shape[1]))
    for i, (c, A, _) in enumerate(peff):
        P[3 * i:3 * i + 3, 3 * c:3 * c + 3] = A
    return np.vstack([J, P])


def linearize(pkg, orc, prob, L, loss, eff, peff):
    """lm_ref.linearize with the point priors' rows under the extrinsic priors'."""
    A, rv, cost, ok = lr.linearize(pkg, orc, prob, L, loss, eff)
    if peff:
        rq = pt_prior_residuals(L, peff, prob)
        A = pt_append_rows(L, peff, A)
        rv = np.concatenate([rv, rq])
        cost = cost + 0.5 * (rq * rq).sum()
    return A, rv, cost, ok


def lm(pkg, orc, prob, opts, *, priors=None, point_priors=None, const=None, groups=0, loss=TRIVIAL):
    """lm_ref.lm (a copy, see the module docstring) with `point_priors` on the points."""
    kind, a = loss
    L = lr.Layout(prob, const, groups)
    eff = lr.effective(L, priors)
    peff = pt_effective(L, point_priors)
    n = L.n
    work = prob.copy()  # evaluation point
    cand = prob.copy()
    x = L.pack(prob)
    x_norm = np.sqrt((x * x).sum())
    its = []
    state = {}

    def evaluate(p):
        A, rv, cost, ok = linearize(pkg, orc, p, L, loss, eff, peff)
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
               num_free_points=L.np, num_free_ext=L.nc,
               num_residuals=2 * prob.num_obs + 6 * len(eff) + 3 * len(peff))
    x_cost, gmax, ok = evaluate(work)
    out["initial_cost"] = x_cost
    if ok and n == 0:
        out.update(num_iterations=0, termination="CONVERGENCE", message=lr.NO_FREE_MESSAGE, final_cost=x_cost,
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
            rp = lr.prior_residuals(L, eff, cand)
            candidate_cost = candidate_cost + 0.5 * (rp * rp).sum() if np.isfinite(rp).all() else DBL_MAX
        if peff and candidate_cost < DBL_MAX:
            rq = pt_prior_residuals(L, peff, cand)
            candidate_cost = candidate_cost + 0.5 * (rq * rq).sum() if np.isfinite(rq).all() else DBL_MAX
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
def jacobian(pkg, orc, prob, *, priors=None, point_priors=None, const=None, groups=0, loss=TRIVIAL):
    L = lr.Layout(prob, const, groups)
    A, _, cost, _ = linearize(pkg, orc, prob, L, loss, lr.effective(L, priors), pt_effective(L, point_priors))
    return L, A, cost


def cost_and_gradient(pkg, orc, prob, *, priors=None, point_priors=None, const=None, groups=0, loss=TRIVIAL):
    L = lr.Layout(prob, const, groups)
    A, rv, cost, _ = linearize(pkg, orc, prob, L, loss, lr.effective(L, priors), pt_effective(L, point_priors))
    return L, cost, A.T @ rv


def covariance(pkg, orc, prob, *, priors=None, point_priors=None, const=None, groups=0, loss=TRIVIAL):
    """lm_ref.covariance with the point priors' rows; num_effective counts the point priors."""
    L = lr.Layout(prob, const, groups)
    eff = lr.effective(L, priors)
    peff = pt_effective(L, point_priors)
    A, _, cost, _ = linearize(pkg, orc, prob, L, loss, eff, peff)
    rank = czr.rank_test(A, L)
    out = dict(kappa=cr.kappa(A), cost=cost, num_parameters=L.n, num_residuals=A.shape[0], num_free_scalars=L.nz,
               num_effective=len(peff), num_effective_ext=len(eff), layout=L, rank=rank)
    if not rank["deficient"]:
        out.update(czr.blocks(cr.sigma_inv(A), L, prob))
        out["point_cov"][L.const_of] = 0.0
        if L.nz == 0:
            out["ext_full"] = out["cam_full"]
    return out


# ---- the shared prior sets -----------------------------------------------------------------------
SIG_GCP = 1e-3
SIG_ALL = np.array([0.1, 0.01, 0.001])  # graded over two decades
SIG_H = 0.01


def referenced(prob):
    m = np.zeros(prob.points.shape[0], bool)
    m[prob.obs_point] = True
    return np.flatnonzero(m)


def gcp3(prob, truth, which=None):
    """Ground control: I / 1e-3 on the first, the middle and the last referenced point (or `which`),
    the mean at the ground truth `truth` [num_points][3]."""
    ref = referenced(prob)
    pts = np.array([ref[0], ref[len(ref) // 2], ref[-1]]) if which is None else np.asarray(which)
    A = np.repeat((np.eye(3) / SIG_GCP)[None], len(pts), axis=0)
    return pts.astype(np.int32), np.array(truth[pts], float), A


def all_points(prob, seed=11, offset=2.0):
    """A full prior on every referenced point: A = Q D (I + 0.2 G) as prior_ref.pose builds its 6x6,
    D = diag(1 / (0.1, 0.01, 0.001)); mu = start + offset sigma o normal, so the priors pull."""
    rng = np.random.default_rng(seed)
    idx, mu, A = [], [], []
    for p in referenced(prob):
        Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        G = rng.standard_normal((3, 3))
        A.append(Q @ np.diag(1.0 / SIG_ALL) @ (np.eye(3) + 0.2 * G))
        mu.append(prob.points[p] + offset * SIG_ALL * rng.standard_normal(3))
        idx.append(p)
    return np.array(idx, np.int32), np.array(mu).reshape(-1, 3), np.array(A).reshape(-1, 3, 3)


def height(prob, seed=11, which=None):
    """Height-only control (A with two zero rows, 1 / 0.01 on z) on every referenced point or on
    `which`; mu = start + 0.01 o normal."""
    rng = np.random.default_rng(seed)
    pts = referenced(prob) if which is None else np.asarray(which)
    A1 = np.zeros((3, 3))
    A1[2, 2] = 1.0 / SIG_H
    mu = prob.points[pts] + SIG_H * rng.standard_normal((len(pts), 3))
    return pts.astype(np.int32), mu, np.repeat(A1[None], len(pts), axis=0)


def offset_priors(prob, off=0.05, sigma=0.01):
    """noise0's set: I / sigma on every referenced point, every mean `off` away on each axis."""
    pts = referenced(prob)
    return (pts.astype(np.int32), prob.points[pts] + off,
            np.repeat((np.eye(3) / sigma)[None], len(pts), axis=0))


# ---- the shapes ------------------------------------------------------------------------------------
_SYNTH = {  # the generator's arguments of the shapes whose ground truth the tests need
    "bal40": dict(kind=0, num_cameras=40, num_points=200, obs_per_point=8, seed=5),
    "rig3x5": dict(kind=1, num_arcs=3, num_rings=5, num_points=200, obs_per_point=6, seed=6),
    "B": dict(kind=0, num_cameras=24, num_points=200, obs_per_point=6, seed=8, rot_noise=0.2, trans_noise=0.4,
              point_noise=0.02),
}


def shape(pkg, orc, case):
    if case == "bal40":
        return cr.bal40(pkg, ())      # gauge-free: camera 0 constant alone
    if case == "rig3x5":
        return cr.rig3x5(pkg, ())     # gauge-free: arc 0 constant alone
    if case == "bal170":
        return cr.bal170(pkg)
    if case == "A":
        return ir.shape_a(pkg, orc)
    if case == "noise0":
        return noise0(pkg)
    return pr.CASES[case](pkg)


def truth(pkg, case):
    """The generator's true points of a shape (its point noise is drawn last: point_noise = 0 changes
    nothing else)."""
    return pkg.synth(**dict(_SYNTH[case], point_noise=0.0)).points


def noise0(pkg):
    """The small rig (4 arcs x 6 rings, 200 points x 6) with noise-free observations at the true
    parameters: the observations' cost is rounding, the priors' cost is everything."""
    return pkg.synth(kind=1, num_arcs=4, num_rings=6, num_points=200, obs_per_point=6, seed=7, rot_noise=0.0,
                     trans_noise=0.0, point_noise=0.0, pixel_noise=0.0)


def make_priors(pkg, prob, case, pset):
    if pset == "gcp3":
        return gcp3(prob, truth(pkg, case))
    if pset == "all":
        return all_points(prob)
    if pset == "all-s14":
        return all_points(prob, seed=14, offset=3.0)
    if pset == "height":
        return height(prob)
    if pset == "offset":
        return offset_priors(prob)
    raise KeyError(pset)


# (name, case, point-prior set, extrinsic-prior set, constant mask, loss, groups, iterations, freeze_camera)
TRAJECTORIES = [
    ("bal40-gcp3", "bal40", "gcp3", None, None, None, 0, 25, False),
    ("rig3x5-gcp3", "rig3x5", "gcp3", None, None, None, 0, 25, False),
    ("B-all", "B", "all", None, None, None, 0, 25, False),
    ("B-height", "B", "height", None, None, None, 0, 25, False),
    ("B-all-freeze", "B", "all", None, None, None, 0, 25, True),
    ("B-all-third-cauchy", "B", "all", None, "third", pr.CAUCHY2, 0, 15, False),
    ("B-all-pose", "B", "all", "pose", None, None, 0, 25, False),
    ("R-all", "R", "all", None, None, None, 0, 25, False),
    ("Bragged-all", "Bragged", "all-s14", None, None, None, 0, 25, False),
    ("A-all-groups7", "A", "all", None, None, None, 7, 25, False),
    ("bal170-all", "bal170", "all", None, None, None, 0, 5, False),
    ("noise0", "noise0", "offset", None, None, None, 0, 10, False),
]
# The choice of cases follows the reference's own spread between two observation orders
# (tests/test_ptprior_ref.py asserts it: cost 1e-10, parameters 1e-8, ten times below the GPU
# tolerances). The higher-noise rig R2 of ptconst_ref cannot serve with free points: with `all` the
# reference differs from itself by 1.4e-9 to 8e-8 of the cost there (prior seeds 11-14), as
# ptconst_ref.case_r2 notes for mixed masks; the rig is covered by R, rig3x5, A and noise0, rejected
# steps by the B cases. On the ragged shape seed 11 gives 1.0e-10, seed 14 with a 3 sigma offset
# 7.4e-12.
REJECTED = ("B-all", "B-height", "B-all-freeze", "B-all-pose", "Bragged-all")  # with rejected steps
TRAJ = {t[0]: t for t in TRAJECTORIES}


def traj_id(t):
    return t[0]


def make_case(pkg, orc, t):
    """(problem, point priors, extrinsic priors or None, constant mask or None, loss, groups,
    iterations) of a trajectory."""
    _, case, pset, eset, mask, loss, groups, iters, freeze = t
    prob = shape(pkg, orc, case)
    ext_priors = qr.PRIORS[eset](prob) if eset else None  # before freeze_camera empties the free set
    prob.freeze_camera = bool(freeze)
    m = pr.MASKS[mask](prob) if mask else None
    return prob, make_priors(pkg, prob, case, pset), ext_priors, m, loss or TRIVIAL, groups, iters
