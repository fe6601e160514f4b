"""Pins tests/lm_ref.py with constant points, the reference of the constant-point tests, on the
cases of tests/ptconst_ref.py (CPU only).

  * with an empty mask lm() is lm() without a mask, record for record and bit for bit (what the
    loop without the feature returned is pinned by tests/test_lm_ref.py);
  * constant points never move, and their count leaves num_parameters / num_free_points;
  * the reference's own spread: on every case of the GPU trajectory test, the given observation
    order and its reverse (intr_ref.reorder) give the same records, every iteration's cost within
    1e-10 relative and the parameters within 1e-8 (the rule of tests/test_intr_ref.py). That is
    what entitles the GPU tests to the project's bounds (cost 1e-9, parameters 1e-7);
  * no free parameter at all: Ceres' "No non-constant parameter blocks found" summary;
  * the covariance arrays: zero rows for constant points, and one constant point repairs the
    gauge-free problems' rank.
The entry points' refusals that need no device are here too."""
import ctypes as C

import numpy as np
import pytest

import cov_ref as cr
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
        base = pr.CASES[case](pkg)
        p = base.copy() if order == 0 else ir.reorder(base)
        m = pr.MASKS[mask](p)
        out = lr.lm(pkg, orc, p, _opts(pkg, iters), const=m, loss=loss or (rr.TRIVIAL, 1.0))
        _cache[key] = (out, p, base, m)
    return _cache[key]


@pytest.mark.parametrize("case,loss", [("B", None), ("R", pr.CAUCHY2)])
def test_empty_mask_is_robust_ref(pkg, orc, case, loss):
    loss = loss or (rr.TRIVIAL, 1.0)
    pa, pb = pr.CASES[case](pkg), pr.CASES[case](pkg)
    a = lr.lm(pkg, orc, pa, _opts(pkg, 8), loss=loss)
    b = lr.lm(pkg, orc, pb, _opts(pkg, 8), const=np.zeros(pb.points.shape[0], bool), loss=loss)
    assert a == b                       # every record and every summary field, bit for bit
    assert len(a["iterations"]) > 3
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)


@pytest.mark.parametrize("t", pr.TRAJECTORIES, ids=pr.traj_id)
def test_constant_points_never_move(pkg, orc, t):
    out, p, base, m = _lm(pkg, orc, t)
    np.testing.assert_array_equal(p.points[m], base.points[m])
    assert out["num_free_points"] == int((~m).sum())
    assert out["num_parameters"] == 3 * out["num_free_points"] + 6 * out["num_free_ext"]
    assert out["final_cost"] < out["initial_cost"]
    if not m.all():
        assert np.abs(p.points[~m] - base.points[~m]).max() > 1e-6
    assert np.abs(p.ext - base.ext).max() > 1e-6


@pytest.mark.parametrize("t", pr.TRAJECTORIES + [pr.RAGGED], ids=pr.traj_id)
def test_two_observation_orders_agree(pkg, orc, t):
    """The reference's own spread, per case (measured: see the printed line; the largest is
    B-third at 3.5e-11 of the cost)."""
    a, pa, _, _ = _lm(pkg, orc, t)
    b, pb, _, _ = _lm(pkg, orc, t, order=1)
    assert a["termination"] == b["termination"] and a["num_iterations"] == b["num_iterations"]
    assert [(i["success"], i["valid"]) for i in a["iterations"]] == [(i["success"], i["valid"]) for i in b["iterations"]]
    ca = np.array([i["cost"] for i in a["iterations"]])
    cb = np.array([i["cost"] for i in b["iterations"]])
    print("orders", pr.traj_id(t), "iterations", a["num_iterations"], "rejected", a["num_unsuccessful_steps"],
          a["termination"], "cost", (np.abs(ca - cb) / np.abs(ca)).max(), "points", np.abs(pa.points - pb.points).max(),
          "ext", np.abs(pa.ext - pb.ext).max())
    assert (np.abs(ca - cb) <= 1e-10 * np.abs(ca)).all()
    assert np.abs(pa.points - pb.points).max() <= 1e-8 and np.abs(pa.ext - pb.ext).max() <= 1e-8


def test_rejected_steps_where_the_gpu_tests_rely_on_them(pkg, orc):
    assert _lm(pkg, orc, ("B", "third", None, 25))[0]["num_unsuccessful_steps"] > 0
    assert _lm(pkg, orc, ("R2", "all", None, 25))[0]["num_unsuccessful_steps"] > 0


def test_free_intrinsics_layout(pkg, orc):
    """Constant points beside free intrinsics: the intrinsic columns keep every observation."""
    prob = ir.shape_a(pkg, orc)
    m = pr.every_third(prob)
    L0, L = lr.Layout(prob, None, 7), lr.Layout(prob, m, 7)
    assert (L.np, L.nc, L.nz) == (L0.np - int(m[L0.pt_of].sum()), L0.nc, L0.nz)
    assert (L.zcol >= 0).sum() == (L0.zcol >= 0).sum()
    assert (L.col[m[prob.obs_point], :3] == -1).all() and (L.col[~m[prob.obs_point], :3] >= 0).all()
    base = prob.copy()
    out = lr.lm(pkg, orc, prob, _opts(pkg, 6), const=m, groups=7)
    np.testing.assert_array_equal(prob.points[m], base.points[m])
    assert out["num_parameters"] == L.n and np.abs(prob.intr - base.intr).max() > 1e-3


def test_no_free_parameter(pkg, orc):
    prob = pr.case_b(pkg)
    prob.freeze_camera = True
    base = prob.copy()
    out = lr.lm(pkg, orc, prob, _opts(pkg), const=True)
    assert (out["termination"], out["num_iterations"], out["iterations"]) == ("CONVERGENCE", 0, [])
    assert out["message"] == lr.NO_FREE_MESSAGE and out["initial_cost"] == out["final_cost"] > 0.0
    assert out["num_parameters"] == 0
    np.testing.assert_array_equal(prob.points, base.points)
    np.testing.assert_array_equal(prob.ext, base.ext)


def test_covariance_blocks_and_gauge(pkg, orc):
    """One constant point takes the gauge-free problems from deficient to well conditioned, and
    its row of point_cov is exactly 0; an empty mask is no mask."""
    for name, make in (("bal40", lambda: cr.bal40(pkg, ())), ("rig3x5", lambda: cr.rig3x5(pkg, ()))):
        prob = make()
        m = np.zeros(prob.points.shape[0], bool)
        free = lr.covariance(pkg, orc, prob, const=None)
        m[0] = True
        one = lr.covariance(pkg, orc, prob, const=m)
        print(name, "camera ratio", free["rank"]["camera_ratio"], "->", one["rank"]["camera_ratio"], "kappa",
              free["kappa"], "->", one["kappa"])
        assert free["rank"]["deficient"] and not one["rank"]["deficient"]
        assert one["rank"]["camera_ratio"] > 1e-3 and one["kappa"] < 1e6
        assert (one["point_cov"][0] == 0.0).all() and np.isfinite(one["point_cov"][1:]).all()
        assert one["num_parameters"] == free["num_parameters"] - 3
    prob = cr.bal40(pkg)
    a, b = lr.covariance(pkg, orc, prob), lr.covariance(pkg, orc, prob, const=None)
    for k in ("point_cov", "ext_cov"):
        np.testing.assert_array_equal(a[k], b[k])
    np.testing.assert_array_equal(a["ext_full"], b["cam_full"])
    # every point constant: Sigma_cc is blockwise U^-1 for a BAL shape
    allc = lr.covariance(pkg, orc, prob, const=True)
    off = allc["cam_full"].copy()
    for c in range(allc["ext_cov"].shape[0]):
        off[6 * c:6 * c + 6, 6 * c:6 * c + 6] = 0.0
    assert np.abs(off).max() == 0.0 and (allc["point_cov"] == 0.0).all()


def test_null_handle_needs_no_device(pkg):
    lib = pkg.load_library()
    m = (C.c_uint8 * 4)(1, 0, 1, 0)
    n = C.c_int32(7)
    assert lib.dab_set_points_constant(None, m) == pkg.DAB_E_INVALID
    assert lib.dab_set_points_constant(None, None) == pkg.DAB_E_INVALID
    assert lib.dab_get_points_constant(None, m, C.byref(n)) == pkg.DAB_E_INVALID
    assert n.value == 7 and list(m) == [1, 0, 1, 0]
    assert "null handle" in pkg.last_error()
