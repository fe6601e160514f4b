"""TEST INFRASTRUCTURE ONLY: the reference for the free-intrinsics tests (a plain module).

oracle/ restates the reference's solve with constant intrinsics (sfm.cc:60-62) and cannot grow
intrinsic columns, so the self-calibrating LM is pinned here:
  * jz(): the six analytic columns d r / d (cx, cy, f0, f1, k0, k1) of every observation in
    numpy, for every (nf, nk), single and composed observations (checked against central
    differences of the oracle's residual in tests/test_intr_ref.py);
  * lm(): robust_ref.lm with the parameter layout extended by the active intrinsic scalars
    after the extrinsics: the same float64 loop and dense Cholesky, statement by statement.
    Its own summation order shows on one shape: with per-camera intrinsics and all groups free
    the problem is weakly constrained, a one-ulp difference in an early step grows about 2.5
    times per iteration, and over 15 iterations two listings of the same problem differ by
    0.9e-10 .. 1.7e-10 of the cost (five orders tried; 4e-13 or less on the other shapes). That
    is the float64 uncertainty of any implementation on that shape, the code under test included.
Also the shapes the CPU and GPU tests share.
"""
import numpy as np

import robust_ref as rr

CENTER, FOCAL, DISTORTION = 1, 2, 4
DBL_MAX = rr.DBL_MAX


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


class _Layout(rr._Layout):
    """robust_ref's layout, then the active scalars of the free intrinsics in (index, slot) order."""

    def __init__(self, prob, groups):
        super().__init__(prob)
        self.n_pc = self.n
        self.act = active_mask(prob, groups)
        self.zi, self.zk = np.nonzero(self.act)
        self.nz = len(self.zi)
        zcol = -np.ones(self.act.shape, np.int64)
        zcol[self.zi, self.zk] = self.n_pc + np.arange(self.nz)
        self.zcol = zcol[prob.obs_intr]  # [N][6]
        self.n = self.n_pc + self.nz

    def pack(self, prob):
        return np.concatenate([super().pack(prob), prob.intr[self.zi, self.zk]])

    def unpack(self, x, prob):
        prob.points[self.pt_of] = x[:3 * self.np].reshape(-1, 3)
        prob.ext[self.ext_of] = x[3 * self.np:self.n_pc].reshape(-1, 6)
        prob.intr[self.zi, self.zk] = x[self.n_pc:]

    def dense(self, J, Jz):
        N = J.shape[0]
        A = np.zeros((2 * N, self.n))
        o, k = np.nonzero(self.col >= 0)
        c = self.col[o, k]
        A[2 * o, c] = J[o, 0, k]
        A[2 * o + 1, c] = J[o, 1, k]
        o, k = np.nonzero(self.zcol >= 0)
        c = self.zcol[o, k]
        A[2 * o, c] = Jz[o, 0, k]
        A[2 * o + 1, c] = Jz[o, 1, k]
        return A


def lm(pkg, orc, prob, opts, groups=0, loss=(rr.TRIVIAL, 1.0)):
    """robust_ref.lm with the active intrinsic scalars of `groups` as unknowns, in place on
    prob.points / prob.ext / prob.intr. Returns a dict shaped like core.summary_to_dict."""
    kind, a = loss
    L = _Layout(prob, groups)
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
        J21 = np.concatenate([J, jz(p)], axis=2)
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
