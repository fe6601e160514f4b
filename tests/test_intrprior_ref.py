"""Pins tests/intrprior_ref.py, the reference of the intrinsic-prior tests (CPU only).

  * intrprior_ref.lm is a copy of lm_ref.lm over groups of linear residual blocks: with
    intr_priors=None it returns ptprior_ref.lm's dict bit for bit, with extrinsic priors, point
    priors, a mask, a loss and free intrinsics; a prior on a constant or unreferenced intrinsic, or
    under freeze_camera, is bit for bit no prior;
  * the priors' part of the gradient equals central differences of the priors' cost on its own, and
    the whole gradient those of the whole cost (1e-6, test_prior_ref.py's step and bound);
  * values in the inactive columns of A and the inactive entries of mu change nothing, bitwise, and
    neither does the order the priors are set in; a block-diagonal A is the sum of its three parts;
  * per trajectory case of the GPU tests: the iteration and rejection counts the issue that asked
    for the priors recorded with its own probe; the reference's own spread between two observation
    orders (intr_ref.reorder) is at most 1e-10 of every iteration's cost and 1e-8 of the parameters,
    ten times below the GPU tests' bounds; and the case is at least 100 of those tolerances away
    from its no-prior trajectory, so a library that ignored the priors cannot pass;
  * the thin-camera covariance case is rank deficient without priors and passes with them.
The entry points' refusals that need no device are here too."""
import ctypes as C

import numpy as np
import pytest

import intr_ref as ir
import intrprior_ref as zr
import lm_ref as lr
import ptprior_ref as ppr


def _opts(pkg, iters=25):
    return pkg.options(max_num_iterations=iters, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)


# ---- the copy is ptprior_ref.lm -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B-all-pose", "B-all-third-cauchy", "A-all-groups7", "R-all", "B-height"])
def test_no_intr_priors_is_ptprior_ref(pkg, orc, name):
    t = ppr.TRAJ[name]
    _, pp, ep, m, loss, groups, iters = ppr.make_case(pkg, orc, t)
    iters = min(iters, 8)
    pa, pb = ppr.make_case(pkg, orc, t)[0], ppr.make_case(pkg, orc, t)[0]
    a = ppr.lm(pkg, orc, pa, _opts(pkg, iters), priors=ep, point_priors=pp, const=m, groups=groups, loss=loss)
    b = zr.lm(pkg, orc, pb, _opts(pkg, iters), priors=ep, point_priors=pp, intr_priors=None, const=m, groups=groups,
              loss=loss)
    assert a == b                       # every record and every summary field, bit for bit
    assert len(a["iterations"]) > 3
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)
    np.testing.assert_array_equal(pa.intr, pb.intr)
    ca = ppr.covariance(pkg, orc, pa, priors=ep, point_priors=pp, const=m, groups=groups, loss=loss)
    cb = zr.covariance(pkg, orc, pb, priors=ep, point_priors=pp, const=m, groups=groups, loss=loss)
    assert ca["cost"] == cb["cost"] and ca["num_residuals"] == cb["num_residuals"]
    if not ca["rank"]["deficient"]:
        for k in ("point_cov", "ext_cov", "cam_full"):
            np.testing.assert_array_equal(ca[k], cb[k])


def _ignored_cases(pkg, orc):
    base = ir.shape_b(pkg, orc)
    drop = 7
    base = base.subset(base.obs_intr != drop).copy()   # intrinsic 7 is referenced by no observation
    g = np.full(base.intr.shape[0], 7)
    g[[2, 3]] = 0                                       # 2 and 3 stay constant
    named = np.array([3, drop, 2], np.int32)
    ip = (named, base.intr[named] + 0.5, np.repeat(np.eye(6)[None] * 3.0, 3, axis=0))
    full = zr.calib(base, 7)
    frozen = base.copy()
    frozen.freeze_camera = True
    return [("constant-and-unreferenced", base, g, ip), ("all-constant-mask", base, 0, full),
            ("freeze-camera", frozen, 7, full)]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_ignored_priors_are_no_priors(pkg, orc, which):
    name, base, g, ip = _ignored_cases(pkg, orc)[which]
    pa, pb = base.copy(), base.copy()
    a = zr.lm(pkg, orc, pa, _opts(pkg, 6), groups=g)
    b = zr.lm(pkg, orc, pb, _opts(pkg, 6), intr_priors=ip, groups=g)
    assert a == b and a["num_residuals"] == 2 * base.num_obs, name
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)
    np.testing.assert_array_equal(pa.intr, pb.intr)
    r, cost = zr.intr_prior_residuals(base, ip, g)
    assert cost == 0.0 and not r.any()


# ---- the gradient ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,g,pset", [("A", 7, "calib"), ("B", 7, "calib"), ("A", [5, 0, 2], "calib"),
                                         ("B", 7, "dist_only")])
def test_gradient_is_central_differences_of_the_cost(pkg, orc, case, g, pset):
    prob = zr.shape(pkg, orc, case)
    groups = zr.case_groups(prob, g)
    ip = zr.PRIORS[pset](prob, groups)
    L, cost, grad = zr.cost_and_gradient(pkg, orc, prob, intr_priors=ip, groups=groups)
    gz = grad[L.n_pc:]
    gp = gz - zr.cost_and_gradient(pkg, orc, prob, groups=groups)[2][L.n_pc:]  # the priors' own part
    worst = worst_p = 0.0
    for j, (i, k) in enumerate(zip(L.zi, L.zk)):
        h = 1e-6 * max(1.0, abs(prob.intr[i, k]))
        hi, lo = prob.copy(), prob.copy()
        hi.intr[i, k] += h
        lo.intr[i, k] -= h
        h2 = hi.intr[i, k] - lo.intr[i, k]
        fd = (zr.cost_and_gradient(pkg, orc, hi, intr_priors=ip, groups=groups)[1]
              - zr.cost_and_gradient(pkg, orc, lo, intr_priors=ip, groups=groups)[1]) / h2
        fd_p = (zr.intr_prior_residuals(hi, ip, groups)[1] - zr.intr_prior_residuals(lo, ip, groups)[1]) / h2
        worst = max(worst, abs(fd - gz[j]) / max(1.0, abs(gz[j])))
        worst_p = max(worst_p, abs(fd_p - gp[j]) / max(1.0, abs(gp[j])))
    print("gradient", case, g, pset, "worst relative difference", worst, "priors' part", worst_p,
          "max |prior gradient|", np.abs(gp).max())
    assert worst <= 1e-6 and worst_p <= 1e-6
    assert np.abs(gp).max() > 1.0  # and the prior is a real part of it


# ---- inactive slots, order, block-diagonal A ------------------------------------------------------
def _run(pkg, orc, prob, ip, groups, iters=5):
    p = prob.copy()
    out = zr.lm(pkg, orc, p, _opts(pkg, iters), intr_priors=ip, groups=groups)
    _, J, cost = zr.jacobian(pkg, orc, p, intr_priors=ip, groups=groups)  # at the end point
    return out, p, (J, cost, zr.cost_and_gradient(pkg, orc, p, intr_priors=ip, groups=groups)[2])


def _assert_same(a, b):
    assert a[0] == b[0]
    for k in ("points", "ext", "intr"):
        np.testing.assert_array_equal(getattr(a[1], k), getattr(b[1], k))
    assert a[2][1] == b[2][1]
    np.testing.assert_array_equal(a[2][0], b[2][0])
    np.testing.assert_array_equal(a[2][2], b[2][2])


@pytest.mark.parametrize("g", [7, [5, 0, 2]])
def test_inactive_columns_and_entries_change_nothing(pkg, orc, g):
    """shape_a: nf = [1, 2, 1], nk = [2, 1, 0]; with groups [5, 0, 2] the mask adds inactive slots."""
    prob = ir.shape_a(pkg, orc)
    groups = zr.case_groups(prob, g)
    idx, mu, A = zr.calib(prob, groups)
    act = lr.Layout(prob, None, groups).act[idx]
    assert (~act).any() and act.any()
    rng = np.random.default_rng(5)
    mu2, A2 = mu.copy(), A.copy()
    mu2[~act] = 1e6 * rng.standard_normal((~act).sum())
    for j in range(len(idx)):
        A2[j][:, ~act[j]] = 1e3 * rng.standard_normal((6, (~act[j]).sum()))
    _assert_same(_run(pkg, orc, prob, (idx, mu, A), groups), _run(pkg, orc, prob, (idx, mu2, A2), groups))


def test_the_order_of_setting_changes_nothing(pkg, orc):
    prob = ir.shape_b(pkg, orc)
    idx, mu, A = zr.calib(prob, 7)
    perm = np.random.default_rng(2).permutation(len(idx))
    assert (perm != np.arange(len(idx))).any()
    _assert_same(_run(pkg, orc, prob, (idx, mu, A), 7), _run(pkg, orc, prob, (idx[perm], mu[perm], A[perm]), 7))


def test_block_diagonal_sqrt_info_is_the_sum_of_three_priors(pkg, orc):
    """Ceres' three NormalPriors on the blocks [1] [2] [3]: their residuals are the block-diagonal
    A's rows, so the cost and the gradient are the three parts' sums."""
    prob = ir.shape_a(pkg, orc)
    idx, mu, A = zr.calib(prob, 7)
    parts = []
    for lo in (0, 2, 4):
        B = np.zeros_like(A)
        B[:, lo:lo + 2, lo:lo + 2] = A[:, lo:lo + 2, lo:lo + 2]
        parts.append(B)
    Abd = parts[0] + parts[1] + parts[2]
    L, c0, g0 = zr.cost_and_gradient(pkg, orc, prob, groups=7)
    _, c, g = zr.cost_and_gradient(pkg, orc, prob, intr_priors=(idx, mu, Abd), groups=7)
    cs = gs = 0.0
    for B in parts:
        _, ck, gk = zr.cost_and_gradient(pkg, orc, prob, intr_priors=(idx, mu, B), groups=7)
        assert ck > c0
        cs, gs = cs + (ck - c0), gs + (gk - g0)
    assert abs((c - c0) - cs) <= 1e-12 * (c - c0)
    assert np.abs((g - g0) - gs).max() <= 1e-12 * np.abs(g - g0).max()
    r, cost = zr.intr_prior_residuals(prob, (idx, mu, Abd), 7)
    assert abs(cost - (c - c0)) <= 1e-12 * cost


# ---- the trajectory cases -------------------------------------------------------------------------
_cache = {}


def _lm(pkg, orc, t, order=0, with_priors=True):
    key = (t[0], order, with_priors)
    if key not in _cache:
        base, ip, ep, pp, m, loss, groups, iters = zr.make_case(pkg, orc, t)
        p = base.copy() if order == 0 else ir.reorder(base)
        out = zr.lm(pkg, orc, p, _opts(pkg, iters), priors=ep, point_priors=pp, intr_priors=ip if with_priors else None,
                    const=m, groups=groups, loss=loss)
        _cache[key] = (out, p, base)
    return _cache[key]


def _intr_diff(a, b):
    return (np.abs(a.intr - b.intr) / np.maximum(1.0, np.abs(a.intr))).max()


@pytest.mark.parametrize("t", zr.TRAJECTORIES, ids=zr.traj_id)
def test_counts_and_two_observation_orders_agree(pkg, orc, t):
    """The recorded iteration / rejection counts, and the reference's own spread, per case (see the
    printed line). Measured worst: cost 1.5e-11 (pcR-calib-s13), parameters 2.1e-10
    (Bcont-cauchy-calib)."""
    a, pa, _ = _lm(pkg, orc, t)
    b, pb, _ = _lm(pkg, orc, t, order=1)
    assert (a["num_iterations"], a["num_unsuccessful_steps"]) == t[-1]
    assert a["termination"] == b["termination"] and a["num_iterations"] == b["num_iterations"]
    assert [(i["success"], i["valid"]) for i in a["iterations"]] == [(i["success"], i["valid"]) for i in b["iterations"]]
    ca = np.array([i["cost"] for i in a["iterations"]])
    cb = np.array([i["cost"] for i in b["iterations"]])
    print("orders", t[0], "iterations", a["num_iterations"], "rejected", a["num_unsuccessful_steps"],
          a["termination"], "cost", (np.abs(ca - cb) / np.abs(ca)).max(), "points", np.abs(pa.points - pb.points).max(),
          "ext", np.abs(pa.ext - pb.ext).max(), "intr", _intr_diff(pa, pb))
    assert (np.abs(ca - cb) <= 1e-10 * np.abs(ca)).all()
    assert np.abs(pa.points - pb.points).max() <= 1e-8 and np.abs(pa.ext - pb.ext).max() <= 1e-8
    assert _intr_diff(pa, pb) <= 1e-8


@pytest.mark.parametrize("t", zr.TRAJECTORIES, ids=zr.traj_id)
def test_priors_change_the_trajectory(pkg, orc, t):
    """At least 100 times the tolerances of the GPU tests (1e-9 on costs, 1e-7 on parameters) in the
    final cost or in the parameters."""
    a, pa, base = _lm(pkg, orc, t)
    b, pb, _ = _lm(pkg, orc, t, with_priors=False)
    rel = abs(a["final_cost"] - b["final_cost"]) / b["final_cost"]
    moved = max(np.abs(pa.points - pb.points).max(), np.abs(pa.ext - pb.ext).max(), _intr_diff(pa, pb))
    print("prior effect", t[0], "final cost", rel, "parameters", moved)
    assert rel > 1e-7 or moved > 1e-5
    assert a["initial_cost"] > b["initial_cost"]
    nfree = len(zr.intr_effective(lr.Layout(base, None, zr.case_groups(base, t[2])), zr.make_case(pkg, orc, t)[1]))
    assert a["num_residuals"] - b["num_residuals"] == 6 * nfree and nfree > 0


def test_the_case_list_covers_what_the_gpu_tests_rely_on(pkg, orc):
    for name in zr.REJECTED:
        assert _lm(pkg, orc, zr.TRAJ[name])[0]["num_unsuccessful_steps"] > 0, name
    counts = {t[0]: len(zr.make_case(pkg, orc, t)[1][0]) for t in zr.TRAJECTORIES}
    assert counts["C-calib"] == 1 and counts["A-calib"] == 3 and counts["B-calib"] == 12
    assert counts["pcB-first16-calib"] == 16 and counts["B-half"] == 6


# ---- the covariance cases -------------------------------------------------------------------------
@pytest.mark.parametrize("keep", [4, 5])
def test_calibration_priors_cure_a_thin_camera(pkg, orc, keep):
    prob, groups, ip = zr.thin_camera(pkg, keep)
    free = zr.covariance(pkg, orc, prob, groups=groups)
    cal = zr.covariance(pkg, orc, prob, groups=groups, intr_priors=ip)
    print("thin camera", keep, "camera ratio", free["rank"]["camera_ratio"], "->", cal["rank"]["camera_ratio"], "kappa",
          cal["kappa"])
    assert free["rank"]["deficient"] and not cal["rank"]["deficient"]
    assert cal["rank"]["camera_ratio"] > 1e-6
    assert cal["num_residuals"] == free["num_residuals"] + 96 and cal["num_parameters"] == free["num_parameters"]


@pytest.mark.parametrize("name", zr.COV_CASES)
def test_priors_tighten_the_covariance(pkg, orc, name):
    prob, groups, ip = zr.cov_case(pkg, name)
    free = zr.covariance(pkg, orc, prob, groups=groups)
    cal = zr.covariance(pkg, orc, prob, groups=groups, intr_priors=ip)
    assert not free["rank"]["deficient"] and not cal["rank"]["deficient"]
    for k in ("intr_cov", "ext_cov"):
        vf = np.array([np.diag(x) for x in free[k]])
        vc = np.array([np.diag(x) for x in cal[k]])
        m = vf > 0
        print(name, k, "variance with prior / free", (vc[m] / vf[m]).min(), (vc[m] / vf[m]).max())
        assert (vc[m] <= vf[m] * (1 + 1e-9)).all() and (vc[m] / vf[m]).min() < 0.1
        assert not vc[~m].any()


# ---- hosts that need no device --------------------------------------------------------------------
def test_null_handle_needs_no_device(pkg):
    lib = pkg.load_library()
    idx = (C.c_int32 * 1)(0)
    mu = (C.c_double * 6)(*([1.0] * 6))
    A = (C.c_double * 36)(*([2.0] * 36))
    n, ne = C.c_int32(7), C.c_int32(9)
    cost = C.c_double(3.0)
    assert lib.dab_set_intr_priors(None, 1, idx, mu, A) == pkg.DAB_E_INVALID
    assert "null handle" in pkg.last_error()
    assert lib.dab_set_intr_priors(None, 0, None, None, None) == pkg.DAB_E_INVALID
    assert lib.dab_get_intr_priors(None, C.byref(n), C.byref(ne), idx, mu, A) == pkg.DAB_E_INVALID
    assert lib.dab_eval_intr_priors(None, mu, C.byref(cost)) == pkg.DAB_E_INVALID
    assert (n.value, ne.value, cost.value, list(mu), idx[0]) == (7, 9, 3.0, [1.0] * 6, 0)
