"""Constant points on the GPU (dab_set_points_constant): the mask through dab_solve and the
covariances, and the direct camera step of a problem without free points, against
tests/ptconst_ref.py (pinned by tests/test_ptconst_ref.py, which also measures the reference's own
spread on every case: at most 3.5e-11 of the cost, 2e-14 of the parameters).

Tolerances are the project's: same iteration records and termination, per-iteration
cost 1e-9 relative, parameters 1e-7; PCG run to convergence against EXPLICIT 1e-6 (the rule of
tests/test_gpu_robust.py); covariance blocks 64 kappa 2^-53 max|Sigma| (tests/test_gpu_covariance.py).
Constant points are compared bit for bit everywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_ref as cr
import intr_ref as ir
import lm_ref as lr
import ptconst_ref as pr
import robust_ref as rr

pytestmark = pytest.mark.gpu

TRIVIAL = (rr.TRIVIAL, 1.0)
LOSS_NAME = {rr.TRIVIAL: None, rr.CAUCHY: "cauchy"}


def records(s):
    return [(i["success"], i["valid"]) for i in s["iterations"]]


def costs(s):
    return [i["cost"] for i in s["iterations"]]


def _opts(pkg, iters, lst=None, **kw):
    return pkg.options(max_num_iterations=iters, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR if lst is None else lst, **kw)


def gpu_solve(pkg, prob, const, iters=25, loss=None, groups=0, lst=None, **kw):
    s = pkg.Solver(0)
    try:
        if loss and loss[0] != rr.TRIVIAL:
            s.set_loss(LOSS_NAME[loss[0]], loss[1])
        s.set_problem(prob)
        if np.any(groups):
            s.set_intrinsics_free(groups)
        if const is not None:
            s.set_points_constant(const)
        return s.solve(_opts(pkg, iters, lst, **kw))
    finally:
        s.close()


_ref = {}


def reference(pkg, orc, key, make, mask, iters, loss=None, groups=0):
    """(summary, solved problem, start, mask) of lm_ref.lm, computed once per key, never modified."""
    if key not in _ref:
        start = make()
        p = start.copy()
        m = pr.MASKS[mask](p) if isinstance(mask, str) else mask
        _ref[key] = (lr.lm(pkg, orc, p, _opts(pkg, iters), const=m, groups=groups, loss=loss or TRIVIAL), p, start, m)
    return _ref[key]


def check_against(tag, g, prob, ref, cost_tol=1e-9):
    o, pref, start, m = ref
    err = max((abs(x - y) / abs(y) for x, y in zip(costs(g), costs(o))), default=0.0)
    print(tag, g["termination"], g["num_iterations"], "cost", g["initial_cost"], "->", g["final_cost"], "rejected",
          g["num_unsuccessful_steps"], "assembly", g["schur_assembly"], "max rel cost err", err, "points err",
          np.abs(prob.points - pref.points).max(), "ext err", np.abs(prob.ext - pref.ext).max())
    assert g["termination"] == o["termination"], (g["message"], o["message"])
    assert g["num_iterations"] == o["num_iterations"]
    assert records(g) == records(o)
    assert g["initial_cost"] == pytest.approx(o["initial_cost"], rel=1e-12)
    for x, y in zip(g["iterations"], o["iterations"]):
        assert abs(x["cost"] - y["cost"]) <= cost_tol * abs(y["cost"]), (x, y)
    assert np.abs(prob.points - pref.points).max() < 1e-7
    assert np.abs(prob.ext - pref.ext).max() < 1e-7
    assert (np.abs(prob.intr - pref.intr) <= 1e-7 * np.maximum(1.0, np.abs(pref.intr))).all()
    np.testing.assert_array_equal(prob.points[m], start.points[m])  # bitwise untouched
    assert g["num_parameters"] == o["num_parameters"] and g["num_free_points"] == o["num_free_points"]
    assert g["num_free_ext"] == o["num_free_ext"]


def traj_ref(pkg, orc, t):
    case, mask, loss, iters = t
    return reference(pkg, orc, ("traj",) + tuple(map(str, t)), lambda: pr.CASES[case](pkg), mask, iters, loss)


# ---- 1. trajectories ----------------------------------------------------------------------------
@pytest.mark.parametrize("t", pr.TRAJECTORIES, ids=pr.traj_id)
def test_trajectory_matches_reference(pkg, orc, gpu, t):
    case, mask, loss, iters = t
    ref = traj_ref(pkg, orc, t)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], iters, loss)
    check_against(pr.traj_id(t), g, prob, ref)
    assert len(ref[0]["iterations"]) >= 6
    if (case, mask, loss) in (("B", "third", None), ("R2", "all", None)):
        assert g["num_unsuccessful_steps"] > 0  # rejected steps: the constant points still never move
    want = pkg.DAB_SCHUR_DIRECT if mask == "all" else pkg.DAB_SCHUR_TILES
    assert g["schur_assembly"] == want


@pytest.mark.parametrize("tiles", ["0", "1"])
@pytest.mark.parametrize("t", [pr.TRAJECTORIES[0], pr.TRAJECTORIES[5], pr.TRAJECTORIES[7]], ids=pr.traj_id)
def test_trajectory_both_assemblies(pkg, orc, gpu, t, tiles, monkeypatch):
    """The general masked path through the pair tables and through the block tiles."""
    monkeypatch.setenv("DAB_SCHUR_TILES", tiles)  # read when the handle is created
    ref = traj_ref(pkg, orc, t)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], t[3], t[2])
    check_against(f"{pr.traj_id(t)}/tiles={tiles}", g, prob, ref)
    assert g["schur_assembly"] == int(tiles)


# ---- 2. the direct path against the general masked one ------------------------------------------
ALL_CASES = [t for t in pr.TRAJECTORIES if t[1] == "all"]


@pytest.mark.parametrize("t", ALL_CASES, ids=pr.traj_id)
def test_direct_matches_general_masked_path(pkg, orc, gpu, t, monkeypatch):
    case, mask, loss, iters = t
    start = traj_ref(pkg, orc, t)[2]
    pd, pg = start.copy(), start.copy()
    d = gpu_solve(pkg, pd, True, iters, loss)
    monkeypatch.setenv("DAB_POINTS_DIRECT", "0")
    g = gpu_solve(pkg, pg, True, iters, loss)
    print(pr.traj_id(t), "direct", d["schur_assembly"], d["final_cost"], "general", g["schur_assembly"], g["final_cost"],
          "max rel", max(abs(x - y) / abs(y) for x, y in zip(costs(d), costs(g))))
    assert d["schur_assembly"] == pkg.DAB_SCHUR_DIRECT
    assert g["schur_assembly"] in (pkg.DAB_SCHUR_PAIRS, pkg.DAB_SCHUR_TILES)
    assert records(d) == records(g) and d["termination"] == g["termination"]
    np.testing.assert_allclose(costs(d), costs(g), rtol=1e-9, atol=0)
    assert np.abs(pd.ext - pg.ext).max() < 1e-7
    np.testing.assert_array_equal(pd.points, start.points)
    np.testing.assert_array_equal(pg.points, start.points)
    assert d["num_parameters"] == g["num_parameters"] == 6 * d["num_free_ext"] and d["num_free_points"] == 0
    check_against(pr.traj_id(t) + "/general", g, pg, traj_ref(pkg, orc, t))


def test_auto_takes_the_direct_path(pkg, orc, gpu):
    t = pr.TRAJECTORIES[1]  # B, all
    ref = traj_ref(pkg, orc, t)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, True, t[3], lst=pkg.DAB_LINEAR_SOLVER_AUTO)
    assert g["schur_assembly"] == pkg.DAB_SCHUR_DIRECT
    assert g["linear_solver_type_used"] == pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR
    check_against("B-all/auto", g, prob, ref)
    # PCG asked for explicitly: the general masked path
    p2 = ref[2].copy()
    p = gpu_solve(pkg, p2, True, 5, lst=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG)
    assert p["linear_solver_type_used"] == pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG
    assert p["final_cost"] < p["initial_cost"]
    np.testing.assert_array_equal(p2.points, ref[2].points)


# ---- 3. the pair tables at scale ----------------------------------------------------------------
@pytest.mark.parametrize("mask", ["third", "all"])
def test_bal170(pkg, orc, gpu, mask):
    """168 free cameras (> 160: pair tables by selection, global-memory camera tables); all
    constant: the direct path with three work-groups of blocks."""
    ref = reference(pkg, orc, ("bal170", mask), lambda: cr.bal170(pkg), mask, 5)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], 5)
    check_against(f"bal170/{mask}", g, prob, ref)
    assert g["schur_assembly"] == (pkg.DAB_SCHUR_PAIRS if mask == "third" else pkg.DAB_SCHUR_DIRECT)
    assert g["num_free_ext"] == 168


# ---- 4. ragged tracks ---------------------------------------------------------------------------
def test_ragged_tracks(pkg, orc, gpu):
    ref = traj_ref(pkg, orc, pr.RAGGED)
    start = ref[2]
    cnt = np.bincount(start.obs_point, minlength=start.points.shape[0])
    assert cnt.min() >= 1 and cnt.max() == 6 and len(np.unique(cnt)) > 3  # padding slots, mixed slices
    prob = start.copy()
    g = gpu_solve(pkg, prob, ref[3], 25)
    check_against("ragged/third", g, prob, ref)


# ---- 5. PCG under the mask ----------------------------------------------------------------------
@pytest.mark.parametrize("how", ["stored-y", "matrix-free", "matrix-free-fp32"])
def test_pcg_converged_matches_explicit(pkg, gpu, how, monkeypatch):
    start = pr.case_b_low(pkg)
    m = pr.every_third(start)
    pe, pp = start.copy(), start.copy()
    e = gpu_solve(pkg, pe, m, 5)
    assert e["num_unsuccessful_steps"] == 0
    if how.startswith("stored-y"):
        monkeypatch.setenv("DAB_PCG_MF", "0")
    p = gpu_solve(pkg, pp, m, 5, lst=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG, eta=1e-14,
                  max_linear_solver_iterations=1000, pcg_fp32=int(how.endswith("fp32")))
    want = {"stored-y": 0, "matrix-free": 1, "matrix-free-fp32": 2}[how]
    print(how, "explicit", repr(e["final_cost"]), "pcg", repr(p["final_cost"]), "assembly", p["schur_assembly"],
          "max rel", max(abs(x - y) / abs(y) for x, y in zip(costs(p), costs(e))))
    assert p["schur_assembly"] == want
    assert records(e) == records(p)
    np.testing.assert_allclose(costs(p), costs(e), rtol=1e-6, atol=0)
    np.testing.assert_array_equal(pp.points[m], start.points[m])
    assert p["num_parameters"] == e["num_parameters"] and p["num_free_points"] == int((~m).sum())


# ---- 6. free intrinsics -------------------------------------------------------------------------
@pytest.mark.parametrize("mask", ["third", "all"])
def test_free_intrinsics_with_constant_points(pkg, orc, gpu, mask):
    ref = reference(pkg, orc, ("intr", mask), lambda: ir.shape_a(pkg, orc), mask, 15, groups=7)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], 15, groups=7)
    check_against(f"shape_a/groups 7/{mask}", g, prob, ref)
    assert g["schur_assembly"] in (pkg.DAB_SCHUR_PAIRS, pkg.DAB_SCHUR_TILES)  # never the direct path
    assert np.abs(prob.intr - ref[2].intr).max() > 1e-3
    assert g["num_parameters"] == 3 * g["num_free_points"] + 6 * g["num_free_ext"] + 13


# ---- 7, 8. freeze_camera ------------------------------------------------------------------------
def _frozen_b(pkg):
    p = pr.case_b(pkg)
    p.freeze_camera = True
    return p


def test_freeze_camera_with_partial_mask(pkg, orc, gpu):
    ref = reference(pkg, orc, ("freeze",), lambda: _frozen_b(pkg), "third", 25)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], 25)
    check_against("freeze/third", g, prob, ref)
    assert g["num_free_ext"] == 0 and g["num_parameters"] == 3 * int((~ref[3]).sum())
    np.testing.assert_array_equal(prob.ext, ref[2].ext)


@pytest.mark.parametrize("lst", ["explicit", "pcg", "auto"])
def test_no_free_parameter(pkg, orc, gpu, lst):
    start = _frozen_b(pkg)
    prob = start.copy()
    which = {"explicit": pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, "pcg": pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG,
             "auto": pkg.DAB_LINEAR_SOLVER_AUTO}[lst]
    g = gpu_solve(pkg, prob, True, 25, lst=which)
    o = lr.lm(pkg, orc, start.copy(), _opts(pkg, 25), const=True)
    assert (g["termination"], g["num_iterations"], g["iterations"]) == ("CONVERGENCE", 0, [])
    assert g["message"] == o["message"] == "Function tolerance reached. No non-constant parameter blocks found."
    assert g["initial_cost"] == g["final_cost"] == pytest.approx(o["initial_cost"], rel=1e-12)
    assert (g["num_parameters"], g["num_free_points"], g["num_free_ext"]) == (0, 0, 0)
    np.testing.assert_array_equal(prob.points, start.points)
    np.testing.assert_array_equal(prob.ext, start.ext)


# ---- 9. emptiness, state, errors ----------------------------------------------------------------
COV_KEYS = ("point_cov", "ext_cov", "ext_full")


def _run(pkg, prob, setup, iters=8):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        setup(s)
        out = s.solve(_opts(pkg, iters))
        cov = s.covariance(full=True)
        return out, cov
    finally:
        s.close()


def test_empty_constant_set_is_the_parent_path_bitwise(pkg, gpu):
    base = cr.bal40_ragged(pkg)  # point 0 is referenced by no observation
    assert not (base.obs_point == 0).any()
    npts = base.points.shape[0]
    only_unref = np.zeros(npts, bool)
    only_unref[0] = True
    plain_p = base.copy()
    plain, plain_cov = _run(pkg, plain_p, lambda s: None)
    assert plain_cov["info"]["status"] == "OK"

    def set_then_clear(s):
        s.set_points_constant(True)
        assert s.get_points_constant()[1] == npts - 1
        s.set_points_constant(None)

    for name, setup in (("null", lambda s: s.set_points_constant(None)),
                        ("zeros", lambda s: s.set_points_constant(np.zeros(npts, bool))),
                        ("unreferenced", lambda s: s.set_points_constant(only_unref)),
                        ("cleared", set_then_clear)):
        p = base.copy()
        out, cov = _run(pkg, p, setup)
        assert costs(out) == costs(plain) and records(out) == records(plain), name
        for k in ("num_parameters", "num_free_points", "schur_assembly", "termination", "final_cost"):
            assert out[k] == plain[k], (name, k)
        np.testing.assert_array_equal(p.points, plain_p.points)
        np.testing.assert_array_equal(p.ext, plain_p.ext)
        for k in COV_KEYS:
            np.testing.assert_array_equal(cov[k], plain_cov[k])
        assert cov["info"]["num_parameters"] == plain_cov["info"]["num_parameters"]


def test_mask_state_and_errors(pkg, gpu):
    lib = pkg.load_library()
    start = pr.case_b(pkg)
    npts = start.points.shape[0]
    prob = start.copy()
    m = pr.every_third(start)
    s = pkg.Solver(0)
    try:
        buf = (C.c_uint8 * npts)()
        n = C.c_int32(-1)
        assert lib.dab_set_points_constant(s.h, buf) == -4  # DAB_E_STATE before dab_set_problem
        assert lib.dab_get_points_constant(s.h, buf, C.byref(n)) == -4
        assert lib.dab_set_points_constant(None, buf) == pkg.DAB_E_INVALID
        s.set_problem(prob)
        assert s.get_points_constant()[1] == 0 and not s.get_points_constant()[0].any()
        raw = np.where(m, 200, 0).astype(np.uint8)  # any non-zero byte
        assert lib.dab_set_points_constant(s.h, raw.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        got, cnt = s.get_points_constant()
        assert (got == raw).all() and cnt == int(m.sum())
        assert lib.dab_get_points_constant(s.h, None, None) == 0
        first = s.solve(_opts(pkg, 6))
        assert first["num_free_points"] == int((~m).sum())
        solved = prob.points.copy()
        # kept by dab_update_parameters and dab_set_loss: the same start walks the same path
        s.update_parameters(start.points, start.ext)
        s.set_loss("trivial")
        assert s.get_points_constant()[1] == int(m.sum())
        again = s.solve(_opts(pkg, 6))
        assert costs(again) == costs(first) and again["num_free_points"] == first["num_free_points"]
        np.testing.assert_array_equal(prob.points, solved)
        np.testing.assert_array_equal(prob.points[m], start.points[m])
        # the getter of the parameters on the handle: the constant points bitwise the input
        pts, ext = np.zeros_like(start.points), np.zeros_like(start.ext)
        s.get_parameters(pts, ext)
        np.testing.assert_array_equal(pts[m], start.points[m])
        # reset by dab_set_problem
        p2 = start.copy()
        s.set_problem(p2)
        assert s.get_points_constant()[1] == 0 and not s.get_points_constant()[0].any()
        free = s.solve(_opts(pkg, 6))
        assert free["num_free_points"] == npts and np.abs(p2.points[m] - start.points[m]).max() > 1e-6
    finally:
        s.close()
    # core.solve's switch is the Solver's
    a, b = start.copy(), start.copy()
    ra = pkg.solve(a, max_iteration=6, freeze_points=m, num_threads=4)
    assert costs(ra) == costs(first)
    np.testing.assert_array_equal(a.points, solved)
    rb = pkg.solve(b, max_iteration=6, freeze_points=True, num_threads=4)
    assert rb["schur_assembly"] == pkg.DAB_SCHUR_DIRECT
    np.testing.assert_array_equal(b.points, start.points)


# ---- 10. covariance -----------------------------------------------------------------------------
def _cov(pkg, prob, const, groups=None, solve_first=0):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        if groups is not None:
            s.set_intrinsics_free(groups)
        if const is not None:
            s.set_points_constant(const)
        out = s.covariance(full=True, intrinsics=groups is not None)
        traj = s.solve(_opts(pkg, solve_first)) if solve_first else None
        return out, traj
    finally:
        s.close()


def _check_cov(tag, g, ref, full_key):
    assert g["info"]["status"] == "OK", g["info"]
    m = max(np.nanmax(np.abs(ref["point_cov"])), np.abs(ref["cam_full"]).max())
    bound = 64.0 * ref["kappa"] * cr.EPS * m
    nan = np.isnan(ref["point_cov"])
    assert (np.isnan(g["point_cov"]) == nan).all()
    errs = {"point_cov": np.abs(np.where(nan, 0.0, g["point_cov"] - ref["point_cov"])).max(),
            "ext_cov": np.abs(g["ext_cov"] - ref["ext_cov"]).max(),
            full_key: np.abs(g[full_key] - ref["cam_full"]).max()}
    if "intr_cov" in g:
        errs["intr_cov"] = np.abs(g["intr_cov"] - ref["intr_cov"]).max()
    for k, e in errs.items():
        print(f"{tag}: {k} error {e:.3e} = {e / bound:.3g} of the bound {bound:.3e} (kappa {ref['kappa']:.3g}, "
              f"camera pivot ratio {g['info']['camera_pivot_ratio']:.3g})")
    for k, e in errs.items():
        assert e <= bound, (k, e, bound)
    L = ref["layout"]
    assert (g["point_cov"][L.const_of] == 0.0).all()          # known exactly
    assert g["info"]["num_free_points"] == L.np and g["info"]["num_parameters"] == ref["num_parameters"]
    assert g["info"]["deficient_points"] == 0 and g["info"]["first_deficient_point"] == -1
    assert g["info"]["cost"] == pytest.approx(ref["cost"], rel=1e-12)
    full = g[full_key]
    assert (full == full.T).all()
    for c in range(g["ext_cov"].shape[0]):
        assert (full[6 * c:6 * c + 6, 6 * c:6 * c + 6] == g["ext_cov"][c]).all()


@pytest.mark.parametrize("name", ["bal40", "rig6x20"])
def test_one_constant_point_fixes_the_gauge(pkg, orc, gpu, name):
    prob = (cr.bal40 if name == "bal40" else cr.rig6x20)(pkg, ())
    m = np.zeros(prob.points.shape[0], bool)
    m[0] = True
    free, _ = _cov(pkg, prob.copy(), None)
    assert free["info"]["status"] == "RANK_DEFICIENT" and free["point_cov"] is None
    ref = lr.covariance(pkg, orc, prob, const=m)
    assert not ref["rank"]["deficient"]
    g, traj = _cov(pkg, prob.copy(), m, solve_first=5)
    _check_cov(name + "/point 0 constant", g, ref, "ext_full")
    assert g["info"]["camera_pivot_ratio"] > 1e-3
    # a dab_solve after the covariance walks the trajectory it walks without it, bitwise
    alone = gpu_solve(pkg, prob.copy(), m, 5)
    assert costs(traj) == costs(alone) and records(traj) == records(alone)


def test_covariance_all_points_constant(pkg, orc, gpu):
    """Sigma_cc = U^-1, blockwise for a BAL shape (the general masked route: S = U)."""
    prob = cr.bal40(pkg, ())
    ref = lr.covariance(pkg, orc, prob, const=True)
    g, _ = _cov(pkg, prob.copy(), True)
    _check_cov("bal40/all constant", g, ref, "ext_full")
    ref_pts = np.where(np.isnan(ref["point_cov"]), np.nan, 0.0)
    np.testing.assert_array_equal(g["point_cov"], ref_pts)
    s = pkg.Solver(0)
    try:
        s.set_problem(prob.copy())
        s.bench_eval_pass(True, 1)
        s.sync()
        ug = s.bench_blocks()["ug"]
    finally:
        s.close()
    iu = np.triu_indices(6)
    bound = 64.0 * ref["kappa"] * cr.EPS * np.abs(ref["cam_full"]).max()
    for c in range(ug.shape[0]):
        U = np.zeros((6, 6))
        U[iu] = ug[c, :21]
        U = U + U.T - np.diag(np.diag(U))
        assert np.abs(g["ext_cov"][c] - np.linalg.inv(U)).max() <= bound
    off = g["ext_full"].copy()
    for c in range(ug.shape[0]):
        off[6 * c:6 * c + 6, 6 * c:6 * c + 6] = 0.0
    assert np.abs(off).max() <= bound


def test_covariance_intrinsics_with_a_constant_point(pkg, orc, gpu):
    prob = cr.rig6x20(pkg, ())
    groups = np.array([7, 0, 2, 5, 0, 4])
    assert prob.intr.shape[0] == 6
    m = np.zeros(prob.points.shape[0], bool)
    m[0] = True
    ref = lr.covariance(pkg, orc, prob, const=m, groups=groups)
    assert not ref["rank"]["deficient"]
    g, _ = _cov(pkg, prob.copy(), m, groups)
    _check_cov("rig6x20/mixed free set/point 0 constant", g, ref, "cam_full")
    assert g["info"]["num_free_scalars"] == ref["num_free_scalars"] > 0
    assert (g["intr_index"] == ref["intr_index"]).all()


# ---- 11. two ranks ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["third", "all"])
def test_two_ranks_match_single_handle(gpu, which):
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "scripts", "dist_check.py"), "--device", "0", "--host-collective",
           "--const-points", which, "--iters", "6", "--solvers", "explicit,auto" if which == "all" else "explicit,pcg"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]
    assert '"bal_0"' in p.stdout and '"rig_0"' in p.stdout
    if which == "all":
        assert p.stdout.count('"assembly": [\n   2,\n   2,\n   2\n  ]') == 4, p.stdout[-3000:]


# ---- 12. the C++ host ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rig", "bal"])
def test_dam_set_points_constant(pkg, gpu, kind):
    import importlib

    from golden_util import GOLDEN
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_%s.deeparc" % kind)
    m = host.DeepArcManager()
    m.read(path)
    xyz0, _ = m.points()
    cams0, _ = m.cameras()
    xyz0, cams0 = xyz0.copy(), cams0.copy()
    m.set_points_constant(True)
    g = host.solve(m, max_iteration=10)
    xyz1, _ = m.points()
    cams1, _ = m.cameras()
    assert g["schur_assembly"] == pkg.DAB_SCHUR_DIRECT and g["num_free_points"] == 0
    assert g["final_cost"] < g["initial_cost"]
    assert xyz1.tobytes() == xyz0.tobytes()                     # every point byte-identical
    assert np.abs(cams1 - cams0).max() > 0.0
    # kept across a re-set of the resident problem (freeze_camera changes the constancy): nothing left to refine
    z = host.solve(m, max_iteration=10, freeze_camera=True)
    assert z["num_iterations"] == 0 and "No non-constant parameter blocks" in z["message"]
    # and off again: the points move
    m.set_points_constant(False)
    f = host.solve(m, max_iteration=3)
    assert f["num_free_points"] > 0 and np.abs(m.points()[0] - xyz0).max() > 0.0
