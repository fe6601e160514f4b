"""Pins tests/extsub_ref.py, the reference of the constant-extrinsic-scalar tests (CPU only).

  * with an empty mask its records equal lm_ref.lm's exactly;
  * with all six bits on extrinsic e they equal lm_ref.lm with ext_const[e] = 1 exactly;
  * constant scalars never move (an input of -0.0 keeps its sign) and leave num_parameters;
  * the gauge table: one translation scalar of a second extrinsic takes the gauge-free problems
    from deficient to camera_ratio > 1e-3; a rotation scalar does not;
  * the reference's own spread: on every case of the GPU trajectory test, the given observation
    order and its reverse (intr_ref.reorder) give the same records, every iteration's cost within
    1e-10 relative and the parameters within 1e-9, ten times under the GPU tolerances;
  * a prior on an extrinsic with constant translation keeps all six values in its residual;
  * the covariance arrays: exact-zero rows and columns for the constant scalars.
The entry points' refusals that need no device are here too."""
import ctypes as C

import numpy as np
import pytest

import extsub_ref as xr
import intr_ref as ir
import lm_ref as lr
import ptconst_ref as pr
import robust_ref as rr


def _opts(pkg, iters=25):
    return pkg.options(max_num_iterations=iters, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)


_cache = {}


def _lm(pkg, orc, t, order=0):
    key = (t, order)
    if key not in _cache:
        case, mask, loss, iters = t
        base = xr.CASES[case](pkg)
        p = base.copy() if order == 0 else ir.reorder(base)
        b = xr.MASKS[mask](p)
        out = xr.lm(pkg, orc, p, _opts(pkg, iters), bits=b, loss=loss or lr.TRIVIAL)
        _cache[key] = (out, p, base, b)
    return _cache[key]


@pytest.mark.parametrize("case,loss", [("Blow", None), ("R", xr.CAUCHY2)])
def test_empty_mask_is_lm_ref(pkg, orc, case, loss):
    loss = loss or lr.TRIVIAL
    pa, pb, pc = (xr.CASES[case](pkg) for _ in range(3))
    a = lr.lm(pkg, orc, pa, _opts(pkg, 8), loss=loss)
    b = xr.lm(pkg, orc, pb, _opts(pkg, 8), bits=np.zeros(pb.ext.shape[0], np.uint8), loss=loss)
    c = xr.lm(pkg, orc, pc, _opts(pkg, 8), bits=None, loss=loss)
    assert a == b == c                  # every record and every summary field, bit for bit
    assert len(a["iterations"]) > 3
    for q in (pb, pc):
        np.testing.assert_array_equal(pa.points, q.points)
        np.testing.assert_array_equal(pa.ext, q.ext)
    assert lr.Layout.__name__ == "Layout" and lr.append_rows.__module__ == "lm_ref"  # the binding is undone


@pytest.mark.parametrize("case,e", [("Blow", 5), ("R", 2), ("R", 6)])
def test_all_six_bits_is_ext_const(pkg, orc, case, e):
    pa, pb = xr.CASES[case](pkg), xr.CASES[case](pkg)
    assert pa.ext_const[e] == 0
    pa.ext_const[e] = 1
    bits = np.zeros(pb.ext.shape[0], np.uint8)
    bits[e] = 63
    a = lr.lm(pkg, orc, pa, _opts(pkg, 8))
    b = xr.lm(pkg, orc, pb, _opts(pkg, 8), bits=bits)
    assert b["num_free_ext"] == a["num_free_ext"] + 1 and b["num_parameters"] == a["num_parameters"]
    strip = lambda o: {k: v for k, v in o.items() if k != "num_free_ext"}
    assert strip(a) == strip(b)         # the same columns in the same order: bit for bit
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)


@pytest.mark.parametrize("t", xr.TRAJECTORIES, ids=xr.traj_id)
def test_constant_scalars_never_move(pkg, orc, t):
    out, p, base, b = _lm(pkg, orc, t)
    L = xr.SubLayout(base, None, 0, b)
    held = np.zeros(base.ext.shape, bool)
    held[L.ext_of] = ~L.ext_free
    assert held.any() and (~held[L.ext_of]).any()
    np.testing.assert_array_equal(p.ext[held].view(np.int64), base.ext[held].view(np.int64))
    assert out["num_free_ext"] == L.nc and out["num_free_points"] == L.np
    assert out["num_parameters"] == 3 * L.np + 6 * L.nc - int(held.sum()) == L.n
    assert out["final_cost"] < out["initial_cost"]
    free = np.zeros(base.ext.shape, bool)
    free[L.ext_of] = L.ext_free
    assert np.abs(p.ext[free] - base.ext[free]).max() > 1e-6


def test_negative_zero_keeps_its_sign(pkg, orc):
    prob = xr.CASES["Blow"](pkg)
    bits = xr.trans_all(prob)
    prob.ext[3, 4] = -0.0
    xr.lm(pkg, orc, prob, _opts(pkg, 4), bits=bits)
    assert np.signbit(prob.ext[3, 4]) and prob.ext[3, 4] == 0.0


@pytest.mark.parametrize("t", xr.TRAJECTORIES, ids=xr.traj_id)
def test_two_observation_orders_agree(pkg, orc, t):
    """The reference's own spread, per case (the printed line; extsub_ref's docstring keeps it)."""
    a, pa, _, _ = _lm(pkg, orc, t)
    b, pb, _, _ = _lm(pkg, orc, t, order=1)
    assert a["termination"] == b["termination"] and a["num_iterations"] == b["num_iterations"]
    assert [(i["success"], i["valid"]) for i in a["iterations"]] == [(i["success"], i["valid"]) for i in b["iterations"]]
    ca = np.array([i["cost"] for i in a["iterations"]])
    cb = np.array([i["cost"] for i in b["iterations"]])
    print("orders", xr.traj_id(t), "iterations", a["num_iterations"], "rejected", a["num_unsuccessful_steps"],
          a["termination"], "cost", (np.abs(ca - cb) / np.abs(ca)).max(), "ext", np.abs(pa.ext - pb.ext).max(),
          "points", np.abs(pa.points - pb.points).max())
    assert (np.abs(ca - cb) <= 1e-10 * np.abs(ca)).all()
    assert np.abs(pa.points - pb.points).max() <= 1e-9 and np.abs(pa.ext - pb.ext).max() <= 1e-9


def test_rejected_steps_where_the_gpu_tests_rely_on_them(pkg, orc):
    assert _lm(pkg, orc, ("Blow", "trans-all", None, 25))[0]["num_unsuccessful_steps"] > 0
    assert _lm(pkg, orc, ("R", "mix", None, 25))[0]["num_unsuccessful_steps"] > 0


@pytest.mark.parametrize("name", sorted(xr.GAUGE))
def test_gauge_table(pkg, orc, name):
    make, e, k = xr.GAUGE[name]
    prob = make(pkg)
    free, kfree = xr.rank(pkg, orc, prob)
    trans, ktrans = xr.rank(pkg, orc, prob, bits=xr.one_bit(prob, e, k))
    rot, _ = xr.rank(pkg, orc, prob, bits=xr.one_bit(prob, e, 0))
    print(name, "camera ratio", free["camera_ratio"], "->", trans["camera_ratio"], "(bit", k, ") rotation bit 0:",
          rot["camera_ratio"], "kappa", kfree, "->", ktrans)
    assert free["deficient"] and rot["deficient"] and not trans["deficient"]
    assert trans["camera_ratio"] > 1e-3 and ktrans < 1e6 < kfree


def test_covariance_zero_rows_and_columns(pkg, orc):
    make, e, k = xr.GAUGE["bal40"]
    prob = make(pkg)
    bits = xr.one_bit(prob, e, k)
    bits[7] = xr.ROTATION
    ref = xr.covariance(pkg, orc, prob, bits=bits)
    L = ref["layout"]
    held = np.flatnonzero(~L.ext_free.ravel())
    assert len(held) == 4 and ref["num_parameters"] == 3 * L.np + 6 * L.nc - 4
    full = ref["ext_full"]
    assert (full[held] == 0.0).all() and (full[:, held] == 0.0).all()
    rest = np.setdiff1d(np.arange(full.shape[0]), held)
    assert (np.diag(full)[rest] > 0.0).all() and np.allclose(full, full.T, rtol=1e-9, atol=0.0)
    c = int(np.flatnonzero(L.ext_of == e)[0])
    assert (ref["ext_cov"][c][k] == 0.0).all() and ref["ext_cov"][c][0, 0] > 0.0
    # an empty mask is lm_ref.covariance
    prob = xr.GAUGE["bal40"][0](pkg)
    prob.ext_const[1] = 1
    a, b = lr.covariance(pkg, orc, prob), xr.covariance(pkg, orc, prob, bits=0)
    for key in ("point_cov", "ext_cov", "ext_full"):
        np.testing.assert_array_equal(a[key], b[key])
    assert a["kappa"] == b["kappa"] and a["num_parameters"] == b["num_parameters"]


def test_prior_keeps_all_six_values(pkg, orc):
    """A prior on an extrinsic with constant translation: the constant scalars enter the residual
    through the offset A_t (t - mu_t); their columns of A are not in the Jacobian."""
    prob = xr.CASES["Blow"](pkg)
    e = 5
    rng = np.random.default_rng(3)
    A = np.eye(6) * 20.0 + rng.normal(size=(6, 6))
    mu = prob.ext[e] + 0.01 * rng.normal(size=6)
    priors = (np.array([e], np.int32), mu[None], A[None])
    bits = np.zeros(prob.ext.shape[0], np.uint8)
    bits[e] = xr.TRANSLATION
    L, J, cost = xr.jacobian(pkg, orc, prob, bits=bits, priors=priors)
    L0, J0, cost0 = lr.jacobian(pkg, orc, prob, priors=priors)
    assert cost == cost0 and J.shape == (J0.shape[0], J0.shape[1] - 3)
    np.testing.assert_array_equal(J, J0[:, L.keep])
    c = int(np.flatnonzero(L.ext_of == e)[0])
    np.testing.assert_array_equal(J[-6:, 3 * L.np + 6 * c - 0:][:, :3], A[:, :3])  # (no constant column before e's)
    base = prob.copy()
    out = xr.lm(pkg, orc, prob, _opts(pkg, 6), bits=bits, priors=priors)
    np.testing.assert_array_equal(prob.ext[e, 3:], base.ext[e, 3:])
    assert out["num_residuals"] == 2 * prob.num_obs + 6 and np.abs(prob.ext[e, :3] - base.ext[e, :3]).max() > 1e-6


def test_no_free_parameter(pkg, orc):
    prob = pr.case_b_low(pkg)
    base = prob.copy()
    out = xr.lm(pkg, orc, prob, _opts(pkg), bits=63, const=True)
    assert (out["termination"], out["num_iterations"], out["iterations"]) == ("CONVERGENCE", 0, [])
    assert out["message"] == lr.NO_FREE_MESSAGE and out["initial_cost"] == out["final_cost"] > 0.0
    assert out["num_parameters"] == 0 and out["num_free_ext"] == 23
    np.testing.assert_array_equal(prob.points, base.points)
    np.testing.assert_array_equal(prob.ext, base.ext)


def test_null_handle_needs_no_device(pkg):
    lib = pkg.load_library()
    b = (C.c_uint8 * 4)(7, 0, 56, 0)
    n = C.c_int32(9)
    assert lib.dab_set_ext_scalars_constant(None, b) == pkg.DAB_E_INVALID
    assert lib.dab_set_ext_scalars_constant(None, None) == pkg.DAB_E_INVALID
    assert lib.dab_get_ext_scalars_constant(None, b, C.byref(n)) == pkg.DAB_E_INVALID
    assert n.value == 9 and list(b) == [7, 0, 56, 0]
    assert "null handle" in pkg.last_error()
    assert (pkg.DAB_EXT_ROTATION, pkg.DAB_EXT_TRANSLATION) == (7, 56)
