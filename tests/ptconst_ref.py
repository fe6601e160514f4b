"""TEST INFRASTRUCTURE ONLY: the reference for the constant-point tests (a plain module).

The reference's solve() keeps `//problem.SetParameterBlockConstant(parameter_block[0]); //freeze
point3d` commented out (sfm.cc:59); the library's switch for it is dab_set_points_constant. Ceres
removes constant blocks from the program it minimises, so the reference here is the LM of
robust_ref / intr_ref over a layout in which constant points get no columns:
  * _Layout: intr_ref._Layout (robust_ref._Layout plus the active intrinsic scalars) with the
    columns of the constant points taken out; their observations keep their rows and their
    camera and intrinsic columns;
  * lm(): the trust-region loop of intr_ref.lm, statement by statement, over that layout (with
    groups = 0 and an empty mask it is robust_ref.lm: tests/test_ptconst_ref.py pins that). No
    free parameter at all gives Ceres' "No non-constant parameter blocks found" summary;
  * covariance(): cov_ref / cov_intr_ref's arrays over that layout, rows of constant points
    exactly 0 (known exactly), unreferenced points NaN.
Also the cases and masks the CPU and GPU tests share.
"""
import numpy as np

import cov_intr_ref as czr
import cov_ref as cr
import intr_ref as ir
import robust_ref as rr

DBL_MAX = rr.DBL_MAX
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


class _Layout(ir._Layout):
    """intr_ref's layout without the columns of the constant points. const_of: the referenced
    constant points (unreferenced flagged points are ignored, as unreferenced blocks are)."""

    def __init__(self, prob, const=None, groups=0):
        super().__init__(prob, groups)
        cm = as_mask(prob, const)
        keep = ~cm[self.pt_of]
        self.const_of = self.pt_of[~keep]
        np_old, np_new = self.np, int(keep.sum())
        # old column -> new column (-1: dropped)
        new_pt = -np.ones(np_old, np.int64)
        new_pt[keep] = np.arange(np_new)
        cmap = np.empty(self.n + 1, np.int64)
        cmap[-1] = -1  # col == -1 stays -1
        pcols = np.arange(3 * np_old)
        cmap[:3 * np_old] = np.where(new_pt[pcols // 3] >= 0, 3 * new_pt[pcols // 3] + pcols % 3, -1)
        cmap[3 * np_old:self.n] = np.arange(3 * np_old, self.n) - 3 * (np_old - np_new)
        self.col = cmap[self.col]
        self.zcol = cmap[self.zcol]
        self.pt_of = self.pt_of[keep]
        self.np = np_new
        self.n_pc = 3 * np_new + 6 * self.nc
        self.n = self.n_pc + self.nz


def lm(pkg, orc, prob, opts, const=None, groups=0, loss=(rr.TRIVIAL, 1.0)):
    """intr_ref.lm with the points of `const` held constant, in place on prob.points / prob.ext /
    prob.intr. Returns a dict shaped like core.summary_to_dict."""
    kind, a = loss
    L = _Layout(prob, const, groups)
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


# ---- covariance ---------------------------------------------------------------------------------
def jacobian(pkg, orc, prob, const=None, groups=0, loss=(rr.TRIVIAL, 1.0)):
    """(layout, dense [2 N][n] Jacobian of the loss-corrected rows, 0.5 sum rho)."""
    r, J = orc.eval_jacobians(pkg, prob)
    J21 = np.concatenate([J, ir.jz(prob)], axis=2)
    _, Jt, ps = rr.correct(loss[0], loss[1], r, J21)
    L = _Layout(prob, const, groups)
    return L, L.dense(Jt[:, :, :15], Jt[:, :, 15:]), 0.5 * ps.sum()


def covariance(pkg, orc, prob, const=None, groups=0, loss=(rr.TRIVIAL, 1.0)):
    """cov_intr_ref.reference over the layout without the constant points: the arrays of
    dab_covariance_intrinsics (with groups = 0: intr_cov empty, cam_full = dab_covariance's
    ext_full), point_cov rows of the referenced constant points exactly 0."""
    L, A, cost = jacobian(pkg, orc, prob, const, groups, loss)
    out = czr.blocks(cr.sigma_inv(A), L, prob)
    out["point_cov"][L.const_of] = 0.0
    out.update(kappa=cr.kappa(A), cost=cost, num_parameters=L.n, num_residuals=A.shape[0], num_free_scalars=L.nz,
               layout=L, rank=cr.rank_test(A, type("N", (), dict(np=L.np, nc=L.nc + int(L.nz > 0)))()))
    return out


# ---- the cases of the constant-point tests ------------------------------------------------------
def case_b(pkg):
    """BAL-shaped: 24 cameras, 200 points x 6 (rejected steps)."""
    return pkg.synth(kind=0, num_cameras=24, num_points=200, obs_per_point=6, seed=8, rot_noise=0.2,
                     trans_noise=0.4, point_noise=0.02)


def case_b_low(pkg):
    """B's base at lower noise (no rejected steps): the PCG comparisons."""
    return pkg.synth(kind=0, num_cameras=24, num_points=200, obs_per_point=6, seed=8, rot_noise=0.1,
                     trans_noise=0.2, point_noise=0.01)


def case_r(pkg):
    """Rig: 4 arcs x 6 rings, 200 points x 6."""
    return pkg.synth(kind=1, num_arcs=4, num_rings=6, num_points=200, obs_per_point=6, seed=7, rot_noise=0.1,
                     trans_noise=0.2, point_noise=0.01)


def case_r2(pkg):
    """The rig at higher noise (rejected steps): all-constant masks only. With mixed masks the
    reference differs from itself by up to 3e-2 between two observation orders at rot >= 0.15."""
    return pkg.synth(kind=1, num_arcs=4, num_rings=6, num_points=200, obs_per_point=6, seed=8, rot_noise=0.15,
                     trans_noise=0.3, point_noise=0.02)


def case_b_ragged(pkg):
    """B's base with tracks of 2-6 observations (padding slots, slices with mixed lanes). The
    generator's seed is 5 (cov_ref.bal40_ragged's), chosen by the reference's own spread between
    two observation orders with every third point constant, 25 iterations: 1.7e-11 of the cost
    (seeds 1, 2, 3: 2.9e-11, 1.3e-11, 2.4e-12). With seed 8 one rejected candidate has cost 2.2e35
    (a point next to a camera's plane) and the reference differs from itself by 1.3e-7 there: a
    parity test on that listing would pin nothing."""
    return rr._ragged(case_b(pkg), np.random.default_rng(5), 2, 6)


def every_third(prob):
    m = np.zeros(prob.points.shape[0], bool)
    m[::3] = True
    return m


def all_points(prob):
    return np.ones(prob.points.shape[0], bool)


def all_but_first5(prob):
    m = np.ones(prob.points.shape[0], bool)
    m[:5] = False
    return m


MASKS = {"third": every_third, "all": all_points, "allbut5": all_but_first5}
CASES = {"B": case_b, "R": case_r, "R2": case_r2, "Bragged": case_b_ragged}
RAGGED = ("Bragged", "third", None, 25)
CAUCHY2 = (rr.CAUCHY, 2.0)
# (case, mask, loss, max_num_iterations): the trajectories of the issue's table
TRAJECTORIES = [
    ("B", "third", None, 25), ("B", "all", None, 25), ("B", "allbut5", None, 25),
    ("B", "third", CAUCHY2, 15), ("B", "all", CAUCHY2, 15),
    ("R", "third", None, 25), ("R", "all", None, 25), ("R", "third", CAUCHY2, 15),
    ("R2", "all", None, 25),
]


def traj_id(t):
    return f"{t[0]}-{t[1]}" + ("-cauchy" if t[2] else "")
