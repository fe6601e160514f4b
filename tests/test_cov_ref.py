"""CPU tests of the covariance reference (tests/cov_ref.py) and of the part of dab_covariance's
C ABI that needs no device. The GPU tests (test_gpu_covariance.py) trust cov_ref only because
these pin it: the inverse of the Jacobi-scaled normal matrix against the SVD pseudo-inverse of
the Jacobian, and the rank test against the shapes known to be gauge-free."""
import ctypes as C

import numpy as np
import pytest

import cov_ref as cr
import lm_ref as lr
import robust_ref as rr

LOSSY = [("bal40", (rr.CAUCHY, 0.5)), ("rig6x20", (rr.CAUCHY, 0.5)), ("bal40", (rr.HUBER, 1.0)),
         ("rig6x20", (rr.HUBER, 1.0))]


@pytest.fixture(scope="module")
def jac(pkg, orc):
    cache = {}

    def get(name, loss=(rr.TRIVIAL, 1.0)):
        if (name, loss) not in cache:
            prob = {**cr.WELL_POSED, **cr.DEFICIENT}[name](pkg)
            cache[(name, loss)] = (prob,) + lr.jacobian(pkg, orc, prob, loss=loss)
        return cache[(name, loss)]
    return get


@pytest.mark.parametrize("name,loss", [(n, (rr.TRIVIAL, 1.0)) for n in sorted(cr.WELL_POSED)] + LOSSY)
def test_two_routes_agree(jac, name, loss):
    """inv of the scaled H, unscaled, against pinv(J) pinv(J)^T: 1e-12 of the largest entry."""
    prob, L, A, _ = jac(name, loss)
    a, b = cr.sigma_inv(A), cr.sigma_pinv(A)
    err = np.abs(a - b).max() / np.abs(b).max()
    print(f"{name} {loss}: n = {L.n}, kappa = {cr.kappa(A):.3g}, routes differ by {err:.2e}")
    assert err <= 1e-12
    assert L.n == A.shape[1] and A.shape[0] == 2 * prob.num_obs


@pytest.mark.parametrize("name,n", [("bal40", 228), ("bal170", 1008), ("bal40-ragged", 228), ("rig3x5", 30),
                                    ("rig6x20", 138), ("freeze", 0)])
def test_shapes(jac, name, n):
    prob, L, _, _ = jac(name)
    assert 6 * L.nc == n
    assert L.np == (199 if name == "bal40-ragged" else prob.points.shape[0])


@pytest.mark.parametrize("name", sorted(cr.WELL_POSED))
def test_rank_test_passes_well_posed(jac, name):
    _, L, A, _ = jac(name)
    t = cr.rank_test(A, L)
    print(f"{name}: point ratio min {t['point_ratio'].min():.3g}, camera ratio {t['camera_ratio']}")
    assert not t["deficient"]
    assert t["point_ratio"].min() > 1e-3                       # eight orders above the threshold
    assert t["camera_ratio"] is None or t["camera_ratio"] > 1e-3


@pytest.mark.parametrize("name", sorted(cr.DEFICIENT))
def test_rank_test_flags_gauge_free(jac, name):
    """Only camera / arc 0 constant: the global scale is free, one singular value of J vanishes."""
    _, L, A, _ = jac(name)
    t = cr.rank_test(A, L)
    assert len(t["deficient_points"]) == 0
    assert t["deficient"] and abs(t["camera_ratio"]) <= 1e-11
    sv = np.linalg.svd(A * cr.jacobi_scale(A), compute_uv=False)
    assert sv[-1] <= 1e-6 * sv[0] and sv[-2] > 1e-4 * sv[0]  # exactly one: sv^2 is H's spectrum


def test_rank_test_flags_single_observation_points(pkg, orc):
    prob, _ = rr.bal_small(pkg, orc, contaminated=False)
    L, A, _ = lr.jacobian(pkg, orc, prob)
    t = cr.rank_test(A, L)
    single = np.flatnonzero(np.bincount(prob.obs_point, minlength=prob.points.shape[0]) == 1)
    assert len(single) > 0
    assert sorted(L.pt_of[t["deficient_points"]]) == sorted(single)
    assert np.abs(t["point_ratio"][t["deficient_points"]]).max() <= 1e-12


# ---- the C ABI without a device ---------------------------------------------------------------
def test_covariance_null_handle_is_invalid(pkg):
    lib = pkg.load_library()
    info = pkg.DabCovarianceInfo()
    assert lib.dab_covariance(None, None, None, None, None, C.byref(info)) == pkg.DAB_E_INVALID
    assert "null handle" in pkg.last_error()


def test_covariance_options_defaults(pkg):
    o = pkg.covariance_options()
    assert o.min_pivot_ratio == 1e-10 and o.jacobi_scaling == 1 and o.reserved == 0
    assert pkg.covariance_options(min_pivot_ratio=1e-8).min_pivot_ratio == 1e-8
    with pytest.raises(AttributeError):
        pkg.covariance_options(no_such_field=1)
