"""CPU tests of the robust-loss reference (tests/robust_ref.py, tests/lm_ref.py) and of the part of
the C ABI that needs no device. The GPU tests (test_gpu_robust.py) trust lm_ref.lm only because
these pin it: the loss table against finite differences, and the LM loop against the oracle
(orc_solve, the DENSE_SCHUR restatement) at the TRIVIAL loss."""
import ctypes as C

import numpy as np
import pytest

import lm_ref as lr
import robust_ref as rr

LOSSES = [(rr.HUBER, 1.0), (rr.SOFT_L1, 1.0), (rr.CAUCHY, 0.5), (rr.HUBER, 2.5), (rr.CAUCHY, 3.0)]


@pytest.mark.parametrize("loss", LOSSES + [(rr.TRIVIAL, 1.0)])
def test_loss_at_zero(loss):
    p, p1 = rr.rho(loss[0], loss[1], np.array([0.0]))
    assert p[0] == 0.0 and p1[0] == 1.0


@pytest.mark.parametrize("a", [0.5, 1.0, 2.5])
def test_huber_continuous_at_switch(a):
    b = a * a
    s = np.array([b * (1 - 1e-12), b, b * (1 + 1e-12)])
    p, p1 = rr.rho(rr.HUBER, a, s)
    assert np.abs(p - b).max() <= 4e-12 * b
    assert np.abs(p1 - 1.0).max() <= 4e-12
    assert p1[1] == 1.0  # s == b is the inner branch


@pytest.mark.parametrize("loss", LOSSES)
def test_rho_prime_matches_central_difference(loss):
    kind, a = loss
    s = np.logspace(-6, 6, 12)
    if kind == rr.HUBER:  # keep the stencil off the kink of rho'' at s = b
        s = s[np.abs(s / (a * a) - 1.0) > 1e-2]
    h = 1e-4 * s
    fd = (rr.rho(kind, a, s + h)[0] - rr.rho(kind, a, s - h)[0]) / (2 * h)
    p, p1 = rr.rho(kind, a, s)
    # error of the central difference itself: truncation h^2 |rho'''| / 6 with |rho'''| <=
    # 2 rho' / s^2 for these losses, plus the rounding of the two rho values (formed from
    # terms of size max(b, rho): 1 + s c scaled by b) divided by 2 h
    eps = np.finfo(np.float64).eps
    tol = (h / s) ** 2 * p1 + 4 * eps * np.maximum(a * a, p) / h
    assert (np.abs(fd - p1) <= tol).all(), (np.abs(fd - p1) / tol).max()
    assert (tol <= 1e-4).all()  # the check is not vacuous anywhere on the grid
    assert (np.diff(rr.rho(kind, a, np.logspace(-6, 6, 200))[1]) <= 0).all()  # rho'' <= 0


def _same(a, o, pa, po):
    assert a["termination"] == o["termination"], (a["message"], o["message"])
    assert a["num_iterations"] == o["num_iterations"]
    assert [i["success"] for i in a["iterations"]] == [i["success"] for i in o["iterations"]]
    assert [i["valid"] for i in a["iterations"]] == [i["valid"] for i in o["iterations"]]
    for x, y in zip(a["iterations"], o["iterations"]):
        assert abs(x["cost"] - y["cost"]) <= 1e-9 * abs(y["cost"]), (x, y)
    assert abs(a["final_cost"] - o["final_cost"]) <= 1e-9 * o["final_cost"]
    assert np.abs(pa.points - po.points).max() < 1e-7
    assert np.abs(pa.ext - po.ext).max() < 1e-7


@pytest.mark.parametrize("case", ["bal", "rig", "bal-freeze", "rig-freeze"])
def test_trivial_lm_reproduces_oracle(pkg, orc, case):
    make = rr.bal_small if case.startswith("bal") else rr.rig_small
    prob, _ = make(pkg, orc)
    prob.freeze_camera = case.endswith("freeze")
    # function_tolerance below the default 1e-6: these small problems would stop after three
    # iterations, before any step is rejected
    opts = pkg.options(max_num_iterations=15, num_threads=4, function_tolerance=1e-12,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)
    pa, po = prob.copy(), prob.copy()
    a = lr.lm(pkg, orc, pa, opts)
    o = orc.solve(pkg, po, opts)
    assert len(o["iterations"]) > 3
    _same(a, o, pa, po)


def test_small_problems_have_the_shapes_the_gpu_tests_need(pkg, orc):
    prob, out = rr.bal_small(pkg, orc)
    cnt = np.bincount(prob.obs_point, minlength=200)
    assert prob.points.shape[0] == 200 and prob.ext.shape[0] == 12
    assert cnt.min() == 1 and cnt.max() == 8
    r, _ = orc.eval_residuals(pkg, prob)
    s = (r * r).sum(axis=1)
    assert s.min() < 1e-20 and np.abs(s - 1.0).min() < 1e-9
    assert 0.04 * len(s) <= out.sum() <= 0.06 * len(s)
    rig, _ = rr.rig_small(pkg, orc)
    assert (rig.obs_ext1 >= 0).any() and rig.points.shape[0] == 200


def test_set_loss_null_handle_needs_no_device(pkg):
    lib = pkg.load_library()
    assert lib.dab_set_loss(None, pkg.DAB_LOSS_CAUCHY, 0.5) == pkg.DAB_E_INVALID
    k, a = C.c_int32(7), C.c_double(7.0)
    assert lib.dab_get_loss(None, C.byref(k), C.byref(a)) == pkg.DAB_E_INVALID
    assert (k.value, a.value) == (7, 7.0)


def test_robust_ordering_on_the_cpu(pkg, orc):
    """The premise of the GPU robustness test, on the reference alone: inlier RMS after a
    solve of (a) clean data, no loss <= (c) contaminated, Cauchy(0.5) < (b) contaminated, no
    loss."""
    a, b, c = lr.robust_triplet(pkg, orc)
    assert a <= c < b, (a, c, b)
