"""Pins tests/ptprior_ref.py, the reference of the point-prior tests (CPU only).

  * ptprior_ref.lm is a copy of lm_ref.lm: with point_priors=None it returns lm_ref.lm's dict bit
    for bit, on all ten prior_ref trajectories, a masked case, a Cauchy case and a free-intrinsics
    case; a prior on a constant or unreferenced point is bit for bit no prior;
  * the priors' part of the gradient equals central differences of the priors' cost on its own, and
    the whole gradient those of the whole cost (1e-6, test_prior_ref.py's step and bound);
  * the reference's own spread: on every trajectory case of the GPU tests, the given observation
    order and its reverse (intr_ref.reorder) give the same records, every iteration's cost within
    1e-10 relative and the parameters within 1e-8, ten times below the GPU tests' bounds (cost
    1e-9, parameters 1e-7). Each case also differs from its no-prior trajectory by at least 100 of
    those tolerances, so a library that ignored the priors cannot pass, and some cases have
    rejected steps;
  * noise0: the priors' cost at the start is at least 1e6 times the observations';
  * the gauge-free covariance problems are rank deficient without priors and pass with gcp3.
The sharding helper and the entry points' refusals that need no device are here too."""
import ctypes as C

import numpy as np
import pytest

import intr_ref as ir
import lm_ref as lr
import prior_ref as qr
import ptconst_ref as pr
import ptprior_ref as ppr
import robust_ref as rr


def _opts(pkg, iters=25):
    return pkg.options(max_num_iterations=iters, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)


# ---- the copy is lm_ref.lm ------------------------------------------------------------------------
def _same_as_lm_ref(pkg, orc, make, iters, **kw):
    pa, pb = make(), make()
    a = lr.lm(pkg, orc, pa, _opts(pkg, iters), **kw)
    b = ppr.lm(pkg, orc, pb, _opts(pkg, iters), point_priors=None, **kw)
    assert a == b                       # every record and every summary field, bit for bit
    assert len(a["iterations"]) > 3
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)
    np.testing.assert_array_equal(pa.intr, pb.intr)
    return a, pa


@pytest.mark.parametrize("t", qr.TRAJECTORIES, ids=qr.traj_id)
def test_no_point_priors_is_lm_ref_on_the_extrinsic_prior_cases(pkg, orc, t):
    _, priors, m, loss, groups, iters = qr.make_case(pkg, orc, t)
    _same_as_lm_ref(pkg, orc, lambda: qr.make_case(pkg, orc, t)[0], iters, priors=priors, const=m, groups=groups,
                    loss=loss)


@pytest.mark.parametrize("case,mask,loss,groups", [("B", "third", None, 0), ("R", None, pr.CAUCHY2, 0),
                                                   ("A", None, None, 7)])
def test_no_point_priors_is_lm_ref(pkg, orc, case, mask, loss, groups):
    def make():
        return ir.shape_a(pkg, orc) if case == "A" else pr.CASES[case](pkg)
    m = pr.MASKS[mask](make()) if mask else None
    _same_as_lm_ref(pkg, orc, make, 8, const=m, groups=groups, loss=loss or lr.TRIVIAL)


def test_priors_on_constant_and_unreferenced_points_are_no_priors(pkg, orc):
    base = pr.case_b(pkg)
    drop = 11
    base = base.subset(base.obs_point != drop).copy()   # point 11 is referenced by no observation
    m = pr.every_third(base)
    named = np.concatenate([np.flatnonzero(m)[:5], [drop]]).astype(np.int32)
    pp = (named, base.points[named] + 0.3, np.repeat(np.eye(3)[None] * 50.0, len(named), axis=0))
    pa, pb = base.copy(), base.copy()
    a = ppr.lm(pkg, orc, pa, _opts(pkg, 8), const=m)
    b = ppr.lm(pkg, orc, pb, _opts(pkg, 8), point_priors=pp, const=m)
    assert a == b and a["num_residuals"] == 2 * base.num_obs
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)
    ca = ppr.covariance(pkg, orc, base, const=m)
    cb = ppr.covariance(pkg, orc, base, point_priors=pp, const=m)
    assert cb["num_effective"] == 0 and ca["num_residuals"] == cb["num_residuals"]
    for k in ("point_cov", "ext_cov", "cam_full"):
        np.testing.assert_array_equal(ca[k], cb[k])
    # ... and without point priors the covariance is lm_ref's
    cl = lr.covariance(pkg, orc, base, const=m)
    for k in ("point_cov", "ext_cov", "cam_full"):
        np.testing.assert_array_equal(ca[k], cl[k])


# ---- the gradient ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pset", [("B", "all"), ("R", "all"), ("R", "height")])
def test_gradient_is_central_differences_of_the_cost(pkg, orc, case, pset):
    prob = pr.CASES[case](pkg)
    pp = ppr.make_priors(pkg, prob, case, pset)
    L, cost, g = ppr.cost_and_gradient(pkg, orc, prob, point_priors=pp)
    gpts = g[:3 * L.np].reshape(-1, 3)
    # the priors' own part against the same differences of the priors' cost alone
    gp = gpts - lr.cost_and_gradient(pkg, orc, prob)[2][:3 * L.np].reshape(-1, 3)
    peff = ppr.pt_effective(L, pp)

    def pcost(p):
        r = ppr.pt_prior_residuals(L, peff, p)
        return 0.5 * (r * r).sum()
    h = 1e-6
    worst = worst_p = 0.0
    pts = [0, L.np // 2, L.np - 1]
    for c in pts:
        for k in range(3):
            hi, lo = prob.copy(), prob.copy()
            hi.points[L.pt_of[c], k] += h
            lo.points[L.pt_of[c], k] -= h
            fd = (ppr.cost_and_gradient(pkg, orc, hi, point_priors=pp)[1]
                  - ppr.cost_and_gradient(pkg, orc, lo, point_priors=pp)[1]) / (2 * h)
            fd_p = (pcost(hi) - pcost(lo)) / (2 * h)
            worst = max(worst, abs(fd - gpts[c, k]) / max(1.0, abs(gpts[c, k])))
            worst_p = max(worst_p, abs(fd_p - gp[c, k]) / max(1.0, abs(gp[c, k])))
    print("gradient", case, pset, "worst relative difference", worst, "priors' part", worst_p, "max |prior gradient|",
          np.abs(gp).max())
    assert worst <= 1e-6 and worst_p <= 1e-6
    assert np.abs(gp[pts]).max() > 1.0  # and the prior is a real part of it


# ---- the trajectory cases -------------------------------------------------------------------------
_cache = {}


def _lm(pkg, orc, t, order=0, with_priors=True):
    key = (t[0], order, with_priors)
    if key not in _cache:
        base, pp, ep, m, loss, groups, iters = ppr.make_case(pkg, orc, t)
        p = base.copy() if order == 0 else ir.reorder(base)
        out = ppr.lm(pkg, orc, p, _opts(pkg, iters), priors=ep, point_priors=pp if with_priors else None, const=m,
                     groups=groups, loss=loss)
        _cache[key] = (out, p, base)
    return _cache[key]


@pytest.mark.parametrize("t", ppr.TRAJECTORIES, ids=ppr.traj_id)
def test_two_observation_orders_agree(pkg, orc, t):
    """The reference's own spread, per case (see the printed line). Measured worst: cost 6.3e-11
    (B-height), parameters 1.3e-11 points and 1.7e-10 extrinsics (B-all-third-cauchy), intrinsics
    2.7e-12."""
    a, pa, _ = _lm(pkg, orc, t)
    b, pb, _ = _lm(pkg, orc, t, order=1)
    assert a["termination"] == b["termination"] and a["num_iterations"] == b["num_iterations"]
    assert [(i["success"], i["valid"]) for i in a["iterations"]] == [(i["success"], i["valid"]) for i in b["iterations"]]
    ca = np.array([i["cost"] for i in a["iterations"]])
    cb = np.array([i["cost"] for i in b["iterations"]])
    print("orders", t[0], "iterations", a["num_iterations"], "rejected", a["num_unsuccessful_steps"],
          a["termination"], "cost", (np.abs(ca - cb) / np.abs(ca)).max(), "points", np.abs(pa.points - pb.points).max(),
          "ext", np.abs(pa.ext - pb.ext).max(), "intr", np.abs(pa.intr - pb.intr).max())
    assert (np.abs(ca - cb) <= 1e-10 * np.abs(ca)).all()
    assert np.abs(pa.points - pb.points).max() <= 1e-8 and np.abs(pa.ext - pb.ext).max() <= 1e-8
    assert np.abs(pa.intr - pb.intr).max() <= 1e-8


@pytest.mark.parametrize("t", ppr.TRAJECTORIES, ids=ppr.traj_id)
def test_priors_change_the_trajectory(pkg, orc, t):
    """At least 100 times the tolerances of the GPU tests (1e-9 on costs, 1e-7 on parameters) in the
    cost or in the parameters. Measured: the final cost moves by 3.6e-5 of itself (rig3x5-gcp3, whose
    points move by 7.5e-4) or more, the points by 7.5e-4 or more."""
    a, pa, _ = _lm(pkg, orc, t)
    b, pb, _ = _lm(pkg, orc, t, with_priors=False)
    rel = abs(a["final_cost"] - b["final_cost"]) / b["final_cost"]
    moved = np.abs(pa.points - pb.points).max()
    print("prior effect", t[0], "final cost", rel, "points", moved)
    assert rel > 1e-7 or moved > 1e-5
    assert a["initial_cost"] > b["initial_cost"]
    assert a["num_residuals"] > b["num_residuals"] and (a["num_residuals"] - b["num_residuals"]) % 3 == 0


def test_rejected_steps_where_the_gpu_tests_rely_on_them(pkg, orc):
    for name in ppr.REJECTED:
        assert _lm(pkg, orc, ppr.TRAJ[name])[0]["num_unsuccessful_steps"] > 0, name


def test_noise0_priors_dominate_the_cost(pkg, orc):
    """The case that makes the tile assembly's bound matter: sum |q_p|^2 is bounded by the cost of
    the observations and the point priors, here 7500 against rounding."""
    base, pp, _, _, _, _, _ = ppr.make_case(pkg, orc, ppr.TRAJ["noise0"])
    r, _ = orc.eval_residuals(pkg, base)
    obs = 0.5 * (r * r).sum()
    L = lr.Layout(base)
    rq = ppr.pt_prior_residuals(L, ppr.pt_effective(L, pp), base)
    pri = 0.5 * (rq * rq).sum()
    print("noise0: observations' cost", obs, "priors' cost", pri)
    assert obs > 0.0 and pri >= 1e6 * obs
    assert np.abs(pp[1] - base.points[pp[0]]).max() == pytest.approx(0.05)


@pytest.mark.parametrize("name", ["bal40", "rig3x5"])
def test_ground_control_fixes_the_gauge(pkg, orc, name):
    prob = ppr.shape(pkg, orc, name)
    free = ppr.covariance(pkg, orc, prob)
    pp = ppr.gcp3(prob, ppr.truth(pkg, name))
    three = ppr.covariance(pkg, orc, prob, point_priors=pp)
    print(name, "camera ratio", free["rank"]["camera_ratio"], "-> gcp3", three["rank"]["camera_ratio"], "kappa",
          three["kappa"])
    assert free["rank"]["deficient"] and not three["rank"]["deficient"]
    assert three["rank"]["camera_ratio"] > 1e-6
    assert three["num_residuals"] == free["num_residuals"] + 9 and three["num_parameters"] == free["num_parameters"]
    assert three["cost"] > free["cost"]
    # the truth is the generator's: everything but the points equals the shape's
    t = pkg.synth(**dict(ppr._SYNTH[name], point_noise=0.0))
    np.testing.assert_array_equal(t.obs_xy, prob.obs_xy)
    np.testing.assert_array_equal(t.ext, prob.ext)
    assert 0.0 < np.abs(t.points - prob.points).max() < 0.1


# ---- hosts that need no device --------------------------------------------------------------------
def test_point_sqrt_info_from_sigmas(pkg):
    np.testing.assert_array_equal(pkg.point_sqrt_info_from_sigmas(0.01), np.eye(3) * 100.0)
    a = pkg.point_sqrt_info_from_sigmas((0.1, 0.5, 0.01))
    np.testing.assert_array_equal(a, np.diag([10.0, 2.0, 100.0]))
    b = pkg.point_sqrt_info_from_sigmas((np.inf, None, 0.01), n=3)
    assert b.shape == (3, 3, 3) and (b[:, :2] == 0.0).all()
    np.testing.assert_array_equal(b[1][2], [0.0, 0.0, 100.0])
    with pytest.raises(ValueError):
        pkg.point_sqrt_info_from_sigmas((1.0, 2.0))


def test_shard_point_priors_splits_with_the_points(pkg):
    prob = pr.case_b(pkg)
    pp = ppr.all_points(prob)
    perm = np.random.default_rng(2).permutation(len(pp[0]))
    pp = (pp[0][perm], pp[1][perm], pp[2][perm])
    world = 3
    owner = prob.point_owner(world)
    seen = []
    for rank in range(world):
        idx, mu, A = prob.shard_point_priors(pp, rank, world)
        shard = prob.shard(rank, world)
        assert len(idx) > 0 and (owner[idx] == rank).all()
        assert np.isin(idx, shard.obs_point).all()          # every one is referenced on its rank
        pos = np.array([int(np.flatnonzero(pp[0] == i)[0]) for i in idx])
        assert (np.diff(pos) > 0).all()                     # the order set is kept
        np.testing.assert_array_equal(mu, pp[1][pos])
        np.testing.assert_array_equal(A, pp[2][pos])
        seen.append(idx)
    np.testing.assert_array_equal(np.sort(np.concatenate(seen)), np.sort(pp[0]))
    one = prob.shard_point_priors(pp, 0, 1)
    for x, y in zip(one, pp):
        np.testing.assert_array_equal(x, y)


def test_null_handle_needs_no_device(pkg):
    lib = pkg.load_library()
    idx = (C.c_int32 * 1)(0)
    mu = (C.c_double * 3)(*([1.0] * 3))
    A = (C.c_double * 9)(*([2.0] * 9))
    n, ne = C.c_int32(7), C.c_int32(9)
    cost = C.c_double(3.0)
    assert lib.dab_set_point_priors(None, 1, idx, mu, A) == pkg.DAB_E_INVALID
    assert "null handle" in pkg.last_error()
    assert lib.dab_set_point_priors(None, 0, None, None, None) == pkg.DAB_E_INVALID
    assert lib.dab_get_point_priors(None, C.byref(n), C.byref(ne), idx, mu, A) == pkg.DAB_E_INVALID
    assert lib.dab_eval_point_priors(None, mu, C.byref(cost)) == pkg.DAB_E_INVALID
    assert (n.value, ne.value, cost.value, list(mu), idx[0]) == (7, 9, 3.0, [1.0] * 3, 0)
