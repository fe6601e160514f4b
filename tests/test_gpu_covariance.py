"""dab_covariance on the GPU: Sigma = (J^T J)^-1 at the handle's parameters by the exact Schur
route (undamped point factor, explicit S by pair tables or block tiles, dense Cholesky, the
inverse from the factor on fp64 MFMA, the per-point fold-back), against tests/cov_ref.py
(pinned by tests/test_cov_ref.py).

Accuracy bound, every returned array: max |Sigma_gpu - Sigma_ref| <= 64 kappa 2^-53 m, with
kappa the condition number of the Jacobi-scaled H and m = max |Sigma_ref| (the forward-error
bound of inversion through Cholesky; 64 is the margin for the dimension constant). Each case
prints the achieved ratio to that bound.

Shapes (cov_ref): bal40 (n = 228: tile assembly, 4 blocks of 64 with the last 36 wide), the same
through the pair tables, bal170 (n = 1008: pair tables by selection, 16 blocks, the last 48),
bal40-ragged (padding slots, tracks of 2-8, an unreferenced point), rig3x5 (n = 30 < 64,
composed entries), rig6x20 (n = 138), freeze (no camera: Sigma_pp = V^-1)."""
import numpy as np
import pytest

import cov_ref as cr
import lm_ref as lr
import robust_ref as rr

pytestmark = pytest.mark.gpu

LOSSES = {"cauchy": (rr.CAUCHY, 0.5), "huber": (rr.HUBER, 1.0)}
SHAPES = ["bal40", "bal40-pairs", "bal170", "bal40-ragged", "rig3x5", "rig6x20", "freeze"]
SENTINEL = -12345.0625

_cache = {}


def case(pkg, orc, name, loss=None):
    """(problem, reference) of a shape, computed once and never modified (tests copy)."""
    key = (name, loss)
    if key not in _cache:
        prob = cr.WELL_POSED[name.replace("-pairs", "")](pkg)
        _cache[key] = (prob, lr.covariance(pkg, orc, prob, loss=LOSSES[loss] if loss else (rr.TRIVIAL, 1.0)))
    return _cache[key]


def gpu_cov(pkg, prob, loss=None, full=True, **opts):
    s = pkg.Solver(0)
    try:
        if loss:
            s.set_loss(loss, LOSSES[loss][1])
        s.set_problem(prob)
        out = s.covariance(full=full, **opts)
        out["raw_jacobians"] = s.jacobians()[1] if loss else None
        return out
    finally:
        s.close()


def check_accuracy(name, g, ref):
    assert g["info"]["status"] == "OK", g["info"]
    m = max(np.nanmax(np.abs(ref["point_cov"])), np.abs(ref["ext_full"]).max() if ref["ext_full"].size else 0.0)
    bound = 64.0 * ref["kappa"] * cr.EPS * m
    errs = {}
    nan = np.isnan(ref["point_cov"])
    assert (np.isnan(g["point_cov"]) == nan).all()
    errs["point_cov"] = np.abs(np.where(nan, 0.0, g["point_cov"] - ref["point_cov"])).max()
    errs["ext_cov"] = np.abs(g["ext_cov"] - ref["ext_cov"]).max() if ref["ext_cov"].size else 0.0
    errs["ext_full"] = np.abs(g["ext_full"] - ref["ext_full"]).max() if ref["ext_full"].size else 0.0
    for k, e in errs.items():
        print(f"{name}: {k} error {e:.3e} = {e / bound:.3g} of the bound {bound:.3e} "
              f"(kappa {ref['kappa']:.3g}, m {m:.3g})")
    for k, e in errs.items():
        assert e <= bound, (k, e, bound)
    assert (g["ext_index"] == ref["ext_index"]).all()
    nfe = ref["ext_cov"].shape[0]
    full = g["ext_full"]
    assert full.shape == (6 * nfe, 6 * nfe)
    assert (full == full.T).all()                                   # bitwise symmetric
    for c in range(nfe):
        assert (full[6 * c:6 * c + 6, 6 * c:6 * c + 6] == g["ext_cov"][c]).all()  # bitwise the same blocks
    assert g["info"]["num_parameters"] == ref["num_parameters"]
    assert g["info"]["num_residuals"] == ref["num_residuals"]
    assert g["info"]["cost"] == pytest.approx(ref["cost"], rel=1e-12)


@pytest.mark.parametrize("name", SHAPES)
def test_accuracy(pkg, orc, gpu, name, monkeypatch):
    if name.endswith("-pairs"):
        monkeypatch.setenv("DAB_SCHUR_TILES", "0")
    prob, ref = case(pkg, orc, name)
    g = gpu_cov(pkg, prob.copy())
    check_accuracy(name, g, ref)
    want = {"bal40": 1, "bal40-pairs": 0, "bal170": 0, "bal40-ragged": 1, "rig3x5": 1, "rig6x20": 1}
    if name in want:  # DAB_SCHUR_TILES = 1, DAB_SCHUR_PAIRS = 0
        assert g["info"]["schur_assembly"] == want[name]
    if name == "freeze":
        assert g["info"]["num_free_ext"] == 0 and g["ext_cov"].shape == (0, 6, 6)
    if name == "bal40-ragged":
        assert np.isnan(g["point_cov"][0]).all()


@pytest.mark.parametrize("loss", sorted(LOSSES))
@pytest.mark.parametrize("name", ["bal40", "rig6x20"])
def test_accuracy_under_loss(pkg, orc, gpu, name, loss):
    """The rows are scaled by sqrt(rho') as dab_solve scales them; dab_eval_jacobians stays raw."""
    prob, ref = case(pkg, orc, name, loss)
    g = gpu_cov(pkg, prob.copy(), loss=loss)
    check_accuracy(f"{name}/{loss}", g, ref)
    _, Jraw = orc.eval_jacobians(pkg, prob)
    assert np.abs(g["raw_jacobians"] - Jraw).max() <= 1e-9 * np.abs(Jraw).max()
    plain = case(pkg, orc, name)[1]
    assert abs(ref["cost"] - plain["cost"]) > 0.01 * plain["cost"]  # the loss is active on this data


# ---- rank test: fail closed ---------------------------------------------------------------------
def raw_call(pkg, prob, loss=None):
    """dab_covariance through the bare ABI with sentinel-filled arrays."""
    import ctypes as C
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        info = pkg.DabCovarianceInfo()
        lib = s.lib
        assert lib.dab_covariance(s.h, None, None, None, None, C.byref(info)) == 0
        nfe, npts = info.num_free_ext, prob.points.shape[0]
        arrs = [np.full((npts, 6), SENTINEL), np.full((nfe, 21), SENTINEL), np.full((6 * nfe, 6 * nfe), SENTINEL)]
        ptr = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]
        assert lib.dab_covariance(s.h, None, ptr[0], ptr[1], ptr[2], C.byref(info)) == 0
        return info, arrs
    finally:
        s.close()


@pytest.mark.parametrize("name", sorted(cr.DEFICIENT))
def test_gauge_free_is_rank_deficient(pkg, gpu, name):
    """Only camera / arc 0 constant (the reference's own gauge rule): the scale is free."""
    info, arrs = raw_call(pkg, cr.DEFICIENT[name](pkg))
    assert info.status == 1
    assert info.deficient_points == 0 and info.first_deficient_point == -1
    assert info.camera_pivot_ratio < 1e-10
    for a in arrs:
        assert (a == SENTINEL).all()


def test_single_observation_points_are_rank_deficient(pkg, orc, gpu):
    prob, _ = rr.bal_small(pkg, orc, contaminated=False)
    info, arrs = raw_call(pkg, prob)
    single = np.flatnonzero(np.bincount(prob.obs_point, minlength=prob.points.shape[0]) == 1)
    assert info.status == 1
    assert info.deficient_points == len(single) > 0
    assert info.first_deficient_point == single.min()
    assert not info.point_pivot_ratio_min > 1e-10
    for a in arrs:
        assert (a == SENTINEL).all()
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        out = s.covariance(full=True)
    finally:
        s.close()
    assert out["info"]["status"] == "RANK_DEFICIENT"
    assert out["point_cov"] is None and out["ext_cov"] is None and out["ext_full"] is None


def test_invalid_arguments(pkg, gpu):
    import ctypes as C
    prob = cr.rig3x5(pkg)
    s = pkg.Solver(0)
    try:
        info = pkg.DabCovarianceInfo()
        assert s.lib.dab_covariance(s.h, None, None, None, None, C.byref(info)) == -4   # DAB_E_STATE
        s.set_problem(prob)
        assert s.lib.dab_covariance(s.h, None, None, None, None, None) == pkg.DAB_E_INVALID
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            o = pkg.covariance_options(min_pivot_ratio=bad)
            assert s.lib.dab_covariance(s.h, C.byref(o), None, None, None, C.byref(info)) == pkg.DAB_E_INVALID
    finally:
        s.close()


# ---- state ----------------------------------------------------------------------------------------
def _solve5(pkg, prob, with_cov, solver=None):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        if with_cov:
            assert s.covariance(full=True)["info"]["status"] == "OK"
        kw = {} if solver is None else dict(linear_solver_type=solver)
        return s.solve(pkg.options(max_num_iterations=5, **kw))
    finally:
        s.close()


@pytest.mark.parametrize("name", ["bal40", "rig6x20", "bal170"])
def test_solve_after_covariance_is_bitwise_the_same(pkg, orc, gpu, name):
    base = case(pkg, orc, name)[0]
    a, b = base.copy(), base.copy()
    sa, sb = _solve5(pkg, a, False), _solve5(pkg, b, True)
    assert [i["cost"] for i in sa["iterations"]] == [i["cost"] for i in sb["iterations"]]
    assert len(sa["iterations"]) >= 3
    assert (a.points == b.points).all() and (a.ext == b.ext).all()


@pytest.mark.parametrize("name", ["bal40", "rig3x5", "bal170"])
def test_two_calls_are_bitwise_equal(pkg, orc, gpu, name):
    prob = case(pkg, orc, name)[0].copy()
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        a, b = s.covariance(full=True), s.covariance(full=True)
    finally:
        s.close()
    for k in ("point_cov", "ext_cov", "ext_full"):
        assert (a[k] == b[k]).all(), k


@pytest.mark.parametrize("name", ["bal40", "rig6x20"])
def test_covariance_ignores_the_last_solver(pkg, orc, gpu, name):
    """After a PCG solve and after an exact solve, at the same parameters: bitwise the same."""
    base = case(pkg, orc, name)[0]
    res = []
    for solver in (pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG, pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR):
        prob = base.copy()
        s = pkg.Solver(0)
        try:
            s.set_problem(prob)
            s.solve(pkg.options(max_num_iterations=3, linear_solver_type=solver))
            s.update_parameters(base.points, base.ext)
            res.append(s.covariance(full=True))
        finally:
            s.close()
    for k in ("point_cov", "ext_cov", "ext_full"):
        assert (res[0][k] == res[1][k]).all(), k
    check_accuracy(name, res[0], case(pkg, orc, name)[1])


def test_sanity_at_the_solution(pkg, orc, gpu):
    """After a converged solve 2 cost / dof is O(pixel_noise^2) (the synthesiser's noise is 1 px)
    and every point block is positive definite."""
    prob = case(pkg, orc, "bal40")[0].copy()
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        summ = s.solve(pkg.options(max_num_iterations=50))
        out = s.covariance()
    finally:
        s.close()
    assert summ["termination"] == "CONVERGENCE"
    info = out["info"]
    assert info["status"] == "OK"
    assert info["cost"] == pytest.approx(summ["final_cost"], rel=1e-9)
    sigma2 = 2.0 * info["cost"] / (info["num_residuals"] - info["num_parameters"])
    print(f"sigma^2 = {sigma2:.4f}")
    assert 0.25 < sigma2 < 4.0
    assert (np.linalg.eigvalsh(out["point_cov"]) > 0.0).all()
    assert (np.linalg.eigvalsh(out["ext_cov"]) > 0.0).all()


# ---- two ranks ------------------------------------------------------------------------------------
def test_two_ranks_match_single_handle(pkg, orc, gpu):
    """Host-staged, both ranks on one GPU, on bal40's shape at its synthesised parameters: the
    camera arrays bitwise equal across the ranks, and they and every owner's point rows within
    the accuracy bound (64 kappa 2^-53 max |Sigma|) of the single handle."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tol = 64.0 * case(pkg, orc, "bal40")[1]["kappa"] * cr.EPS
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "scripts", "dist_check.py"), "--device", "0", "--host-collective",
           "--covariance", "--iters", "0", "--cov-tol", repr(tol)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    print(p.stdout[-1500:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]
    assert '"ranks_equal": true' in p.stdout


# ---- host API -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rig", "bal"])
def test_host_manager_covariance(pkg, gpu, kind):
    """DeepArcManager.covariance on the committed tiny scene with one extra constant extrinsic:
    rows as sizes() counts them, values bitwise those of Solver.covariance on the same arrays;
    with the reference's gauge rule alone the scene is rank deficient."""
    import importlib
    import os

    import deeparc_ref
    from golden_util import GOLDEN
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_%s.deeparc" % kind)
    m = host.DeepArcManager()
    m.read(path)
    loose = m.covariance()
    assert loose["info"]["status"] == "RANK_DEFICIENT" and loose["point_cov"] is None
    assert loose["info"]["camera_pivot_ratio"] < 1e-10
    g = m.covariance(extra_const=(1,), full=True)
    assert g["info"]["status"] == "OK"
    sz = m.sizes()
    nfe = sz["extrinsics"] - 2
    assert g["point_cov"].shape == (sz["points"], 3, 3) and g["ext_cov"].shape == (nfe, 6, 6)
    assert g["ext_full"].shape == (6 * nfe, 6 * nfe)
    prob = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    prob.ext_const[1] = 1
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        d = s.covariance(full=True)
    finally:
        s.close()
    for k in ("point_cov", "ext_cov", "ext_full"):
        assert (g[k] == d[k]).all(), k
    assert (g["ext_index"] == d["ext_index"]).all()
    if kind == "rig":  # arcs first, then the rings 1.. (ring 0 shares the identity with arc 0)
        want = [("arc", int(e)) if e < sz["arc"] else ("ring", int(e) - sz["arc"] + 1) for e in d["ext_index"]]
        assert g["ext_label"] == want
