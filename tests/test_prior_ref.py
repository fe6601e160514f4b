"""Pins tests/lm_ref.py with priors, the reference of the extrinsic-prior tests, on the prior sets
and cases of tests/prior_ref.py (CPU only).

  * with no priors, and with a prior on a constant extrinsic alone, lm() is lm() without the
    argument, record for record and bit for bit (what the loop without the feature returned is
    pinned by tests/test_lm_ref.py);
  * the gradient's camera part equals central differences of the reference's cost (1e-6);
  * the reference's own spread: on every trajectory case of the GPU tests, the given observation
    order and its reverse (intr_ref.reorder) give the same records, every iteration's cost within
    1e-10 relative and the parameters within 1e-8. That is what entitles the GPU tests to the
    project's bounds (cost 1e-9, parameters 1e-7). Each case also differs from its no-prior
    trajectory by far more than any tolerance;
  * the gauge-free covariance problems are rank deficient without priors and pass with pos3, and
    with one position prior alone.
The entry points' refusals that need no device are here too."""
import ctypes as C

import numpy as np
import pytest

import cov_ref as cr
import intr_ref as ir
import lm_ref as lr
import prior_ref as qr
import ptconst_ref as pr
import robust_ref as rr


def _opts(pkg, iters=25):
    return pkg.options(max_num_iterations=iters, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)


_cache = {}


def _lm(pkg, orc, t, order=0, with_priors=True):
    key = (t[0], order, with_priors)
    if key not in _cache:
        base, priors, m, loss, groups, iters = qr.make_case(pkg, orc, t)
        p = base.copy() if order == 0 else ir.reorder(base)
        out = lr.lm(pkg, orc, p, _opts(pkg, iters), priors=priors if with_priors else None, const=m, groups=groups,
                    loss=loss)
        _cache[key] = (out, p, base)
    return _cache[key]


@pytest.mark.parametrize("case,mask,loss", [("B", None, None), ("R", "third", pr.CAUCHY2)])
def test_no_priors_is_ptconst_ref(pkg, orc, case, mask, loss):
    loss = loss or (rr.TRIVIAL, 1.0)
    pa, pb, pc = (pr.CASES[case](pkg) for _ in range(3))
    m = pr.MASKS[mask](pa) if mask else None
    a = lr.lm(pkg, orc, pa, _opts(pkg, 8), const=m, loss=loss)
    b = lr.lm(pkg, orc, pb, _opts(pkg, 8), priors=None, const=m, loss=loss)
    assert a == b                       # every record and every summary field, bit for bit
    assert len(a["iterations"]) > 3
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)
    # a prior on a constant extrinsic alone (camera 0 / arc 0) is skipped entirely
    only_const = (np.array([0], np.int32), np.ones((1, 6)), np.eye(6)[None])
    assert pc.ext_const[0]
    c = lr.lm(pkg, orc, pc, _opts(pkg, 8), priors=only_const, const=m, loss=loss)
    assert a == c


@pytest.mark.parametrize("case,pset", [("B", "pose"), ("R", "pose"), ("R", "pos3")])
def test_gradient_is_central_differences_of_the_cost(pkg, orc, case, pset):
    prob = pr.CASES[case](pkg)
    priors = qr.PRIORS[pset](prob)
    L, cost, g = lr.cost_and_gradient(pkg, orc, prob, priors=priors)
    gc = g[3 * L.np:].reshape(-1, 6)
    # the priors' own part (the observations' gradient is ~1e7 times larger and would hide it)
    # against the same differences of the priors' cost alone
    gp = gc - lr.cost_and_gradient(pkg, orc, prob, priors=None)[2][3 * L.np:].reshape(-1, 6)
    eff = lr.effective(L, priors)

    def pcost(p):
        r = lr.prior_residuals(L, eff, p)
        return 0.5 * (r * r).sum()
    h = 1e-6
    worst = worst_p = 0.0
    cams = [int(np.flatnonzero(L.ext_of == e)[0]) for e in priors[0][:4]]
    for c in cams:
        for k in range(6):
            hi, lo = prob.copy(), prob.copy()
            hi.ext[L.ext_of[c], k] += h
            lo.ext[L.ext_of[c], k] -= h
            fd = (lr.cost_and_gradient(pkg, orc, hi, priors=priors)[1]
                  - lr.cost_and_gradient(pkg, orc, lo, priors=priors)[1]) / (2 * h)
            fd_p = (pcost(hi) - pcost(lo)) / (2 * h)
            worst = max(worst, abs(fd - gc[c, k]) / max(1.0, abs(gc[c, k])))
            worst_p = max(worst_p, abs(fd_p - gp[c, k]) / max(1.0, abs(gp[c, k])))
    print("gradient", case, pset, "worst relative difference", worst, "priors' part", worst_p, "max |prior gradient|",
          np.abs(gp).max())
    assert worst <= 1e-6 and worst_p <= 1e-6
    assert np.abs(gp[cams]).max() > 1.0  # and the prior is a real part of it


@pytest.mark.parametrize("t", qr.TRAJECTORIES, ids=qr.traj_id)
def test_two_observation_orders_agree(pkg, orc, t):
    """The reference's own spread, per case (see the printed line)."""
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
    assert a["num_residuals"] == 2 * pa.num_obs + 6 * len(qr.make_case(pkg, orc, t)[1][0])


@pytest.mark.parametrize("t", qr.TRAJECTORIES, ids=qr.traj_id)
def test_priors_change_the_trajectory(pkg, orc, t):
    """At least 100 times the tolerances of the GPU tests (1e-9 on costs, 1e-7 on parameters), so
    that a solve that dropped the priors cannot pass them. Measured: the final cost moves by 2.9e-4
    (R-pose-all) to 3.4 of itself, except on R2-pose-all, where every point is constant at a high
    noise and the cost left after 25 iterations is the points' error: 2.4e-7, with the extrinsics
    2.8e-5 apart."""
    a, pa, _ = _lm(pkg, orc, t)
    b, pb, _ = _lm(pkg, orc, t, with_priors=False)
    rel = abs(a["final_cost"] - b["final_cost"]) / b["final_cost"]
    print("prior effect", t[0], "final cost", rel, "ext", np.abs(pa.ext - pb.ext).max())
    assert rel > 1e-7 and np.abs(pa.ext - pb.ext).max() > 1e-5
    assert a["initial_cost"] > b["initial_cost"]


def test_rejected_steps_where_the_gpu_tests_rely_on_them(pkg, orc):
    for t in qr.TRAJECTORIES:
        if t[0] in qr.REJECTED:
            assert _lm(pkg, orc, t)[0]["num_unsuccessful_steps"] > 0, t[0]


@pytest.mark.parametrize("name", ["bal40", "rig3x5"])
def test_position_priors_fix_the_gauge(pkg, orc, name):
    prob = cr.bal40(pkg, ()) if name == "bal40" else cr.rig3x5(pkg, ())
    free = lr.covariance(pkg, orc, prob, priors=None)
    three = lr.covariance(pkg, orc, prob, priors=qr.pos3(prob, seed=3))
    L = three["layout"]
    one = lr.covariance(pkg, orc, prob, priors=qr.pos3(prob, seed=3, which=[L.ext_of[len(L.ext_of) // 2]]))
    print(name, "camera ratio", free["rank"]["camera_ratio"], "-> pos3", three["rank"]["camera_ratio"], "kappa",
          three["kappa"], "one prior alone", one["rank"]["camera_ratio"])
    assert free["rank"]["deficient"]
    assert not three["rank"]["deficient"] and not one["rank"]["deficient"]
    assert three["rank"]["camera_ratio"] > 1e-6 and one["rank"]["camera_ratio"] > 1e-7
    assert three["kappa"] < 1e8
    assert three["num_residuals"] == free["num_residuals"] + 18 and three["num_parameters"] == free["num_parameters"]
    assert three["cost"] > free["cost"]
    # no priors: the covariance without the argument bit for bit
    well = cr.bal40(pkg) if name == "bal40" else cr.rig3x5(pkg)
    a, b = lr.covariance(pkg, orc, well, const=None), lr.covariance(pkg, orc, well, priors=None)
    for k in ("point_cov", "ext_cov", "cam_full"):
        np.testing.assert_array_equal(a[k], b[k])


def test_sqrt_info_from_sigmas(pkg):
    a = pkg.sqrt_info_from_sigmas(0.02, 0.05)
    np.testing.assert_array_equal(a, np.diag([50.0] * 3 + [20.0] * 3))
    b = pkg.sqrt_info_from_sigmas(None, 0.01, n=3)
    assert b.shape == (3, 6, 6) and (b[:, :3] == 0.0).all()
    np.testing.assert_array_equal(b[1][3:, 3:], np.eye(3) * 100.0)


def test_null_handle_needs_no_device(pkg):
    lib = pkg.load_library()
    idx = (C.c_int32 * 1)(0)
    mu = (C.c_double * 6)(*([1.0] * 6))
    A = (C.c_double * 36)(*([2.0] * 36))
    n, ne = C.c_int32(7), C.c_int32(9)
    cost = C.c_double(3.0)
    assert lib.dab_set_ext_priors(None, 1, idx, mu, A) == pkg.DAB_E_INVALID
    assert "null handle" in pkg.last_error()
    assert lib.dab_set_ext_priors(None, 0, None, None, None) == pkg.DAB_E_INVALID
    assert lib.dab_get_ext_priors(None, C.byref(n), C.byref(ne), idx, mu, A) == pkg.DAB_E_INVALID
    assert lib.dab_eval_ext_priors(None, mu, C.byref(cost)) == pkg.DAB_E_INVALID
    assert (n.value, ne.value, cost.value, list(mu), idx[0]) == (7, 9, 3.0, [1.0] * 6, 0)
