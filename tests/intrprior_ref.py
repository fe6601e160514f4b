"""TEST INFRASTRUCTURE ONLY: the reference, prior sets and cases of the intrinsic-prior tests (a plain module).

A prior on intrinsic i is Ceres' NormalPrior(A, mu) with a NULL loss over that intrinsic's blocks:
the residual block r = A[:, act] (intr[i][act] - mu[act]), A 6x6 over (cx, cy, f0, f1, k0, k1), act
the slots lm_ref.Layout gives a column (the model has them and the groups free them). A prior on an
intrinsic without an active slot (constant, unreferenced, freeze_camera) is skipped entirely, and so
are the inactive columns of an effective one: the library's documented simplification.
num_residuals += 6 per effective prior. lm / jacobian / cost_and_gradient / covariance here take
`intr_priors` = (index [n], mean [n][6], sqrt_info [n][6][6]) beside ptprior_ref's arguments and put
the 6-row blocks under the point priors' rows, at Layout's z columns, in ascending intrinsic index
whatever the order they were set in.

lm() is a THIRD COPY of lm_ref.lm: lm_ref.py and ptprior_ref.py are frozen test files for the change
that added intrinsic priors. It is written over a generic list of linear residual blocks
(columns, A, mu) with r = A (x[columns] - mu), x = Layout.pack: the extrinsic, point and intrinsic
priors are three groups of such blocks, each group's rows and cost added in turn, so that with
intr_priors=None it returns ptprior_ref.lm's dict bit for bit (tests/test_intrprior_ref.py pins
that). The follow-up is to fold the three loops into lm_ref.lm over that block list and delete the
two copies.
"""
import numpy as np

import cov_intr_ref as czr
import cov_ref as cr
import intr_ref as ir
import lm_ref as lr
import prior_ref as qr
import ptconst_ref as pr
import ptprior_ref as ppr
import robust_ref as rr

DBL_MAX = lr.DBL_MAX
TRIVIAL = lr.TRIVIAL


# ---- linear residual blocks ---------------------------------------------------------------------
# A block is (columns [k], A [m][k], mu [k]): the m residuals A (x[columns] - mu) of the free
# parameters x = L.pack(prob). A group is a list of blocks.
def ext_blocks(L, priors):
    """lm_ref.effective as blocks: the priors on free extrinsics, in the order set."""
    return [(3 * L.np + 6 * c + np.arange(6), A, mu) for c, A, mu in lr.effective(L, priors)]


def pt_blocks(L, point_priors):
    """ptprior_ref.pt_effective as blocks: the priors on free points, in the order set."""
    return [(3 * c + np.arange(3), A, mu) for c, A, mu in ppr.pt_effective(L, point_priors)]


def intr_effective(L, intr_priors):
    """The places in `intr_priors` of the effective priors (some active slot), by ascending
    intrinsic index."""
    if intr_priors is None:
        return []
    idx = np.asarray(intr_priors[0])
    return sorted((i for i in range(len(idx)) if L.act[int(idx[i])].any()), key=lambda i: int(idx[i]))


def intr_blocks(L, intr_priors):
    """The effective intrinsic priors as blocks over the active slots' z columns."""
    out = []
    if intr_priors is None:
        return out
    idx, mu, A = intr_priors
    zcol = -np.ones(L.act.shape, np.int64)
    zcol[L.zi, L.zk] = L.n_pc + np.arange(L.nz)
    for i in intr_effective(L, intr_priors):
        act = L.act[int(idx[i])]
        out.append((zcol[int(idx[i])][act], np.asarray(A[i], float)[:, act], np.asarray(mu[i], float)[act]))
    return out


def block_residuals(L, group, prob):
    """The stacked residuals of a group at prob's parameters."""
    if not group:
        return np.zeros(0)
    x = L.pack(prob)
    return np.concatenate([A @ (x[cols] - mu) for cols, A, mu in group])


def block_rows(group, J):
    """The dense Jacobian with the group's rows under it."""
    if not group:
        return J
    rows = []
    for cols, A, _ in group:
        P = np.zeros((A.shape[0], J.shape[1]))
        P[:, cols] = A
        rows.append(P)
    return np.vstack([J] + rows)


def intr_prior_residuals(prob, intr_priors, groups=0):
    """[n][6] residuals in the order set (zero rows for ignored priors) and 0.5 sum |r|^2."""
    L = lr.Layout(prob, None, groups)
    idx = np.asarray(intr_priors[0])
    r = np.zeros((len(idx), 6))
    eff = intr_effective(L, intr_priors)
    for i, (cols, A, mu) in zip(eff, intr_blocks(L, intr_priors)):
        r[i] = A @ (L.pack(prob)[cols] - mu)
    return r, 0.5 * sum((r[i] * r[i]).sum() for i in eff)


def linearize(pkg, orc, prob, L, loss, groups_of_blocks):
    """(A, r, cost, ok): lm_ref.linearize without priors, then every group's rows and cost in turn."""
    A, rv, cost, ok = lr.linearize(pkg, orc, prob, L, loss, [])
    for grp in groups_of_blocks:
        if grp:
            rg = block_residuals(L, grp, prob)
            A = block_rows(grp, A)
            rv = np.concatenate([rv, rg])
            cost = cost + 0.5 * (rg * rg).sum()
    return A, rv, cost, ok


def _groups(L, priors, point_priors, intr_priors):
    return [ext_blocks(L, priors), pt_blocks(L, point_priors), intr_blocks(L, intr_priors)]


def lm(pkg, orc, prob, opts, *, priors=None, point_priors=None, intr_priors=None, const=None, groups=0,
       loss=TRIVIAL):
    """lm_ref.lm (a copy, see the module docstring) over groups of linear residual blocks."""
    kind, a = loss
    L = lr.Layout(prob, const, groups)
    blocks = _groups(L, priors, point_priors, intr_priors)
    n = L.n
    work = prob.copy()  # evaluation point
    cand = prob.copy()
    x = L.pack(prob)
    x_norm = np.sqrt((x * x).sum())
    its = []
    state = {}

    def evaluate(p):
        A, rv, cost, ok = linearize(pkg, orc, p, L, loss, blocks)
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
               num_residuals=2 * prob.num_obs + sum(A.shape[0] for grp in blocks for _, A, _ in grp))
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
        for grp in blocks:
            if grp and candidate_cost < DBL_MAX:
                rg = block_residuals(L, grp, cand)
                candidate_cost = candidate_cost + 0.5 * (rg * rg).sum() if np.isfinite(rg).all() else DBL_MAX
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
def jacobian(pkg, orc, prob, *, priors=None, point_priors=None, intr_priors=None, const=None, groups=0,
             loss=TRIVIAL):
    L = lr.Layout(prob, const, groups)
    A, _, cost, _ = linearize(pkg, orc, prob, L, loss, _groups(L, priors, point_priors, intr_priors))
    return L, A, cost


def cost_and_gradient(pkg, orc, prob, *, priors=None, point_priors=None, intr_priors=None, const=None, groups=0,
                      loss=TRIVIAL):
    L = lr.Layout(prob, const, groups)
    A, rv, cost, _ = linearize(pkg, orc, prob, L, loss, _groups(L, priors, point_priors, intr_priors))
    return L, cost, A.T @ rv


def covariance(pkg, orc, prob, *, priors=None, point_priors=None, intr_priors=None, const=None, groups=0,
               loss=TRIVIAL):
    """ptprior_ref.covariance with the intrinsic priors' rows; num_effective counts them."""
    L = lr.Layout(prob, const, groups)
    blocks = _groups(L, priors, point_priors, intr_priors)
    A, _, cost, _ = linearize(pkg, orc, prob, L, loss, blocks)
    rank = czr.rank_test(A, L)
    out = dict(kappa=cr.kappa(A), cost=cost, num_parameters=L.n, num_residuals=A.shape[0], num_free_scalars=L.nz,
               num_effective=len(blocks[2]), num_effective_pt=len(blocks[1]), num_effective_ext=len(blocks[0]),
               layout=L, rank=rank)
    if not rank["deficient"]:
        out.update(czr.blocks(cr.sigma_inv(A), L, prob))
        out["point_cov"][L.const_of] = 0.0
        if L.nz == 0:
            out["ext_full"] = out["cam_full"]
    return out


# ---- the shared prior sets -----------------------------------------------------------------------
SIG_C, SIG_F, SIG_K = 2.0, 5e-3, 5e-3  # centre in px, focal relative, distortion absolute


def sigmas(k6):
    """(2, 2, 5e-3 |f0|, 5e-3 |f1|, 5e-3, 5e-3) of one intrinsic; a zero is replaced by 1."""
    sig = np.array([SIG_C, SIG_C, SIG_F * abs(k6[2]), SIG_F * abs(k6[3]), SIG_K, SIG_K])
    sig[sig == 0.0] = 1.0
    return sig


def calib(prob, groups, seed=11, offset=1.0):
    """A full prior on every free intrinsic, ascending: A = Q diag(1 / sig) (I + 0.2 G) as
    prior_ref.pose builds its 6x6 (a certificate with correlations), mu = start + offset sig o
    normal."""
    rng = np.random.default_rng(seed)
    L = lr.Layout(prob, None, groups)
    idx, mu, A = [], [], []
    for i in czr.free_intrinsics(L):
        sig = sigmas(prob.intr[i])
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        G = rng.standard_normal((6, 6))
        A.append(Q @ np.diag(1.0 / sig) @ (np.eye(6) + 0.2 * G))
        mu.append(prob.intr[i] + offset * sig * rng.standard_normal(6))
        idx.append(i)
    return np.array(idx, np.int32), np.array(mu).reshape(-1, 6), np.array(A).reshape(-1, 6, 6)


def half(prob, groups, seed=11, offset=1.0):
    """Every second prior of calib."""
    idx, mu, A = calib(prob, groups, seed, offset)
    return idx[::2].copy(), mu[::2].copy(), A[::2].copy()


def focal_cols(prob, groups, seed=11, offset=1.0):
    """calib with only the focal columns 2, 3 of A kept."""
    idx, mu, A = calib(prob, groups, seed, offset)
    B = np.zeros_like(A)
    B[:, :, 2:4] = A[:, :, 2:4]
    return idx, mu, B


def dist_only(prob, groups, seed=11, offset=1.0):
    """A = diag(0, 0, 0, 0, 1 / 5e-3, 1 / 5e-3) on every free intrinsic; mu = start + 5e-3 o normal on
    the distortion slots."""
    rng = np.random.default_rng(seed)
    L = lr.Layout(prob, None, groups)
    idx = czr.free_intrinsics(L)
    A1 = np.diag([0.0, 0.0, 0.0, 0.0, 1.0 / SIG_K, 1.0 / SIG_K])
    mu = prob.intr[idx].copy()
    mu[:, 4:6] += offset * SIG_K * rng.standard_normal((len(idx), 2))
    return idx.astype(np.int32), mu, np.repeat(A1[None], len(idx), axis=0)


PRIORS = {"calib": calib, "half": half, "focal_cols": focal_cols, "dist_only": dist_only}


# ---- the shapes and the trajectories ----------------------------------------------------------------
def shape(pkg, orc, case):
    if case == "A":
        return ir.shape_a(pkg, orc)
    if case == "B":
        return ir.shape_b(pkg, orc)
    if case == "Bcont":
        return ir.shape_b(pkg, orc, contaminated=True)
    if case == "C":
        return ir.shape_c(pkg, orc)
    return pr.CASES[case[3:]](pkg)  # "pc-B", "pc-R": ptconst_ref's shapes


def case_groups(prob, g):
    """An int, a list per intrinsic, or ("first", k): groups 7 on the first k intrinsics."""
    if isinstance(g, tuple):
        return czr.first(prob, g[1])
    return np.asarray(g) if isinstance(g, list) else g


# (name, shape, groups, prior set, seed, offset, extrinsic-prior set, point-prior set, constant mask, loss,
#  iterations, (iterations, rejected steps) of the reference)
TRAJECTORIES = [
    ("A-calib", "A", 7, "calib", 11, 1.0, None, None, None, None, 25, (4, 0)),
    ("A-502-calib", "A", [5, 0, 2], "calib", 11, 1.0, None, None, None, None, 25, (2, 0)),
    ("B-calib", "B", 7, "calib", 11, 1.0, None, None, None, None, 25, (6, 0)),
    ("B-half", "B", 7, "half", 11, 1.0, None, None, None, None, 25, (5, 0)),
    ("B-focal-cols", "B", 7, "focal_cols", 11, 1.0, None, None, None, None, 25, (9, 0)),
    ("B-dist-only", "B", 7, "dist_only", 11, 1.0, None, None, None, None, 25, (25, 0)),
    ("C-calib", "C", 7, "calib", 11, 1.0, None, None, None, None, 25, (3, 0)),
    ("pcR-calib-s13", "pc-R", 7, "calib", 13, 3.0, None, None, None, None, 25, (18, 3)),
    ("pcR-calib-s16", "pc-R", 7, "calib", 16, 3.0, None, None, None, None, 25, (13, 1)),
    ("pcB-first16-calib", "pc-B", ("first", 16), "calib", 11, 1.0, None, None, None, None, 25, (7, 0)),
    ("Bcont-cauchy-calib", "Bcont", 7, "calib", 11, 1.0, None, None, None, pr.CAUCHY2, 15, (15, 0)),
    # the two cases the change that added the priors chose itself (counts measured with this module)
    ("A-calib-pose-allpoints", "A", 7, "calib", 11, 1.0, "pose", "all", None, None, 25, (3, 0)),
    ("pcB-first16-calib-third", "pc-B", ("first", 16), "calib", 11, 1.0, None, None, "third", None, 25, (16, 3)),
]
TRAJ = {t[0]: t for t in TRAJECTORIES}
REJECTED = ("pcR-calib-s13", "pcR-calib-s16", "pcB-first16-calib-third")  # with rejected steps in the reference
# The choice of cases follows the reference's own spread between two observation orders
# (tests/test_intrprior_ref.py asserts it: cost 1e-10, parameters 1e-8). ptconst_ref's R with calib
# seed 14 (1.3e-10 to 1.8e-10 of the cost) and R2 (1e-6) do not qualify. For the every-third mask,
# shape B with all 12 intrinsics free (calib seed 11) walks 24 iterations and differs from itself by
# 7.4e-7 in the parameters; ptconst_ref's B with its first 16 intrinsics free replaces it (4.4e-13
# of the cost, 3.2e-12 in the parameters, three rejected steps).


def traj_id(t):
    return t[0]


def make_case(pkg, orc, t):
    """(problem, intrinsic priors, extrinsic priors or None, point priors or None, constant mask or
    None, loss, groups, iterations) of a trajectory."""
    _, case, g, pset, seed, offset, eset, ptset, mask, loss, iters, _ = t
    prob = shape(pkg, orc, case)
    groups = case_groups(prob, g)
    ip = PRIORS[pset](prob, groups, seed, offset)
    ep = qr.pose(prob, groups=groups) if eset == "pose" else None
    pp = ppr.all_points(prob) if ptset == "all" else None
    m = pr.MASKS[mask](prob) if mask else None
    return prob, ip, ep, pp, m, loss or TRIVIAL, groups, iters


# ---- covariance cases -------------------------------------------------------------------------------
COV_CASES = ("rig3x5-mixed", "rig6x20-mixed-masks", "bal40-first16")
COV_SEED = 3


def cov_case(pkg, name):
    """(problem, groups, calib priors at seed 3) of a cov_intr_ref case."""
    prob, groups = czr.CASES[name](pkg)
    return prob, groups, calib(prob, groups, seed=COV_SEED)


def thin_camera(pkg, keep=4):
    """bal40-first16 with camera 5 cut to its first `keep` observations: 2 keep rows for its 6
    extrinsic and 5 intrinsic unknowns (nf 1, nk 2), rank deficient for the intrinsics alone."""
    prob, groups = czr.CASES["bal40-first16"](pkg)
    of5 = np.flatnonzero(prob.obs_ext0 == 5)
    sel = np.ones(prob.num_obs, bool)
    sel[of5[keep:]] = False
    prob = prob.subset(np.flatnonzero(sel)).copy()
    return prob, groups, calib(prob, groups, seed=COV_SEED)
