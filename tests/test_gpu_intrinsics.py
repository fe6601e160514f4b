"""Free intrinsics (dab_set_intrinsics_free) in the exact Schur LM step, on the GPU. The
reference is tests/intr_ref.py (pinned by tests/test_intr_ref.py: the analytic intrinsic columns
by central differences of the oracle's residual, its LM loop by the oracle at groups = 0, and
its own spread between two observation orders).

Tolerances are the project's bounds between two fp64 evaluations that differ in summation
order: Jacobian entries as test_jacobian_kernel_vs_golden (TOL_JAC = 1e-11 of the largest entry of
each observation's Jacobian), blocks 1e-9 of each array's largest
entry, cost sums 1e-12, per-iteration LM cost 1e-9 relative, points and extrinsics 1e-7,
intrinsics 1e-7 max(1, |reference value|) (focal lengths are about 5e3).

Shapes (intr_ref.shape_a / b / c, all with the intrinsics offset: focal x 1.01, centre by
(+3, -2) px, k0 + 0.01): (a) the 3 x 5 rig with intr_nf = [1, 2, 1], intr_nk = [2, 1, 0]
(composed observations, shared intrinsics, inactive slots); (b) 12 cameras with per-camera
intrinsics and ragged tracks (padding slots, single-observation points, rejected steps); (c)
the same with one intrinsic seen by every camera (eleven masked intrinsics unreferenced); (d)
the contaminated variants of (a) and (b) under Cauchy(0.5)."""
import ctypes as C

import numpy as np
import pytest

import intr_ref as ir
import lm_ref as lr
import robust_ref as rr
from golden_util import TOL_JAC

pytestmark = pytest.mark.gpu

CAUCHY = ("cauchy", 0.5)
LOSS_REF = {None: (rr.TRIVIAL, 1.0), CAUCHY: (rr.CAUCHY, 0.5)}


@pytest.fixture(scope="module")
def shapes(pkg, orc):
    """Never modified: tests copy them."""
    return {"a": ir.shape_a(pkg, orc), "b": ir.shape_b(pkg, orc), "c": ir.shape_c(pkg, orc),
            "da": ir.shape_a(pkg, orc, contaminated=True), "db": ir.shape_b(pkg, orc, contaminated=True)}


def _opts(pkg, iters=15, **kw):
    return pkg.options(max_num_iterations=iters, linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, **kw)


_ref_cache = {}


def reference(pkg, orc, shapes, shape, groups, loss=None, iters=15):
    """lm_ref.lm on a copy of the shape, computed once per case."""
    key = (shape, groups, loss, iters)
    if key not in _ref_cache:
        p = shapes[shape].copy()
        o = pkg.options(max_num_iterations=iters, num_threads=4,
                        linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)
        _ref_cache[key] = (lr.lm(pkg, orc, p, o, groups=groups, loss=LOSS_REF[loss]), p)
    return _ref_cache[key]


def gpu_solve(pkg, prob, groups, loss=None, iters=15, **kw):
    s = pkg.Solver(0)
    try:
        if loss is not None:
            s.set_loss(*loss)
        s.set_problem(prob)
        s.set_intrinsics_free(groups)
        return s.solve(_opts(pkg, iters, **kw))
    finally:
        s.close()


def costs(summary):
    return [it["cost"] for it in summary["iterations"]]


def records(summary):
    return [(it["iteration"], it["success"], it["valid"]) for it in summary["iterations"]]


# ---- 1. Jacobians ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_intrinsic_jacobians_match_reference(pkg, gpu, shapes, shape):
    prob = shapes[shape].copy()
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        J = s.intrinsic_jacobians()
    finally:
        s.close()
    ref = ir.jz(prob)
    assert J.shape == ref.shape == (prob.num_obs, 2, 6)
    # the bound and scaling of test_jacobian_kernel_vs_golden: TOL_JAC of the largest entry of each
    # observation's Jacobian
    scale = np.abs(ref).reshape(len(ref), -1).max(axis=1)
    err = np.abs(J - ref).reshape(len(ref), -1).max(axis=1) / scale
    print("intrinsic Jacobians, largest per-observation relative error", err.max())
    assert err.max() < TOL_JAC, err.max()
    assert (J[:, :, ~ir.struct_mask(prob)[prob.obs_intr].any(axis=0)] == 0).all()
    nf1 = prob.intr_nf[prob.obs_intr] == 1
    assert (J[nf1][:, 1, 2] != 0).all() and (J[nf1][:, :, 3] == 0).all()  # one focal length: both rows


# ---- 2. update ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["a", "b"])
def test_update_intrinsics_then_residuals(pkg, orc, gpu, shapes, shape):
    prob = shapes[shape].copy()
    other = prob.copy()
    other.intr[:, 0] += 1.5
    other.intr[:, 2:4] *= 0.997
    other.intr[:, 4] -= 0.004
    other.intr[:, 5] += 0.002
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        np.testing.assert_array_equal(s.get_intrinsics(), prob.intr)
        s.update_intrinsics(other.intr)
        np.testing.assert_array_equal(s.get_intrinsics(), other.intr)
        r, cost = s.residuals()
    finally:
        s.close()
    ro, _ = orc.eval_residuals(pkg, other)
    np.testing.assert_allclose(r, ro, rtol=0, atol=1e-12 * np.abs(ro).max())
    assert cost == pytest.approx(0.5 * (ro * ro).sum(), rel=1e-12)
    r0, _ = orc.eval_residuals(pkg, prob)
    assert np.abs(ro - r0).max() > 1.0  # the update did change the residuals


# ---- 3. blocks ------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("shape,loss,groups", [("a", None, 7), ("b", None, 7), ("da", CAUCHY, 7), ("db", CAUCHY, 7),
                                               ("a", None, 5)])
def test_intrinsic_blocks_match_host_sums(pkg, orc, gpu, shapes, shape, loss, groups, fused, monkeypatch):
    monkeypatch.setenv("DAB_EVAL_FUSED", fused)
    prob = shapes[shape].copy()
    s = pkg.Solver(0)
    try:
        if loss is not None:
            s.set_loss(*loss)
        s.set_problem(prob)
        s.set_intrinsics_free(groups)
        s.bench_eval_pass(True, 1)
        s.sync()
        zg = s.intrinsic_blocks()
        b = s.bench_blocks()
        r, _ = s.residuals()
        Jz = s.intrinsic_jacobians()
        _, raw_cost = s.residuals()
    finally:
        s.close()
    ref = ir.scaled_intrinsic_blocks(prob, r, Jz, groups, LOSS_REF[loss])
    assert zg.shape == ref.shape and zg.shape[0] == (3 if shape in ("a", "da") else 12)

    def close(x, y):
        scale = np.abs(y).max()
        assert np.abs(x - y).max() <= 1e-9 * scale, (np.abs(x - y).max(), scale)

    close(zg[:, :21], ref[:, :21])
    close(zg[:, 21:], ref[:, 21:])
    if loss is not None:
        assert abs(b["cost"][0] - raw_cost) > 0.1 * raw_cost  # the loss is active on this data
    if groups == 5:
        assert (zg[:, [2, 7, 11, 12]] == 0).all()  # the focal rows and columns are not selected


# ---- 4. trajectories ------------------------------------------------------------------------
def _check_trajectory(pkg, orc, shapes, shape, groups, loss):
    o, pref = reference(pkg, orc, shapes, shape, groups, loss)
    prob = shapes[shape].copy()
    g = gpu_solve(pkg, prob, groups, loss)
    print(shape, groups, loss, g["termination"], g["num_iterations"], "cost", g["initial_cost"], "->", g["final_cost"],
          "rejected", g["num_unsuccessful_steps"],
          "max rel cost err", max(abs(x - y) / abs(y) for x, y in zip(costs(g), costs(o))),
          "intr err", (np.abs(prob.intr - pref.intr) / np.maximum(1.0, np.abs(pref.intr))).max())
    assert g["termination"] == o["termination"], (g["message"], o["message"])
    assert g["num_iterations"] == o["num_iterations"]
    assert records(g) == records(o)
    assert g["initial_cost"] == pytest.approx(o["initial_cost"], rel=1e-12)
    for x, y in zip(g["iterations"], o["iterations"]):
        assert abs(x["cost"] - y["cost"]) <= 1e-9 * abs(y["cost"]), (x, y)
    assert np.abs(prob.points - pref.points).max() < 1e-7
    assert np.abs(prob.ext - pref.ext).max() < 1e-7
    assert (np.abs(prob.intr - pref.intr) <= 1e-7 * np.maximum(1.0, np.abs(pref.intr))).all()
    assert g["num_parameters"] == o["num_parameters"]
    assert len(o["iterations"]) >= 3
    return g, o


@pytest.mark.parametrize("groups", [7, 2, 5])
@pytest.mark.parametrize("shape", ["a", "b", "c"])
def test_lm_trajectory_matches_reference(pkg, orc, gpu, shapes, shape, groups):
    g, o = _check_trajectory(pkg, orc, shapes, shape, groups, None)
    if shape == "b" and groups == 7:
        assert g["num_unsuccessful_steps"] > 0
    if shape == "c":  # eleven of the twelve masked intrinsics are referenced by no observation
        fixed, _ = reference(pkg, orc, shapes, "c", 0)
        assert g["num_parameters"] == fixed["num_parameters"] + {7: 5, 2: 1, 5: 4}[groups]


@pytest.mark.parametrize("shape", ["da", "db"])
def test_lm_trajectory_matches_reference_under_cauchy(pkg, orc, gpu, shapes, shape):
    _check_trajectory(pkg, orc, shapes, shape, 7, CAUCHY)


def test_unreferenced_masked_intrinsics_are_untouched(pkg, gpu, shapes):
    prob = shapes["c"].copy()
    gpu_solve(pkg, prob, 7)
    np.testing.assert_array_equal(prob.intr[1:], shapes["c"].intr[1:])
    assert np.abs(prob.intr[0] - shapes["c"].intr[0]).max() > 0.1


# ---- 5. schedules ---------------------------------------------------------------------------
def _knob_runs(pkg, shapes, shape, monkeypatch, knob, values, iters=10):
    out = []
    for v in values:
        monkeypatch.setenv(knob, v)
        p = shapes[shape].copy()
        out.append((gpu_solve(pkg, p, 7, iters=iters), p))
    return out


def _same_path(a, b, tol=1e-9):
    (ra, pa), (rb, pb) = a, b
    assert records(ra) == records(rb) and ra["termination"] == rb["termination"]
    np.testing.assert_allclose(costs(ra), costs(rb), rtol=tol)
    assert np.abs(pa.points - pb.points).max() < 1e-7 and np.abs(pa.ext - pb.ext).max() < 1e-7
    assert (np.abs(pa.intr - pb.intr) <= 1e-7 * np.maximum(1.0, np.abs(pb.intr))).all()


def _bitwise(a, b):
    (ra, pa), (rb, pb) = a, b
    assert costs(ra) == costs(rb)
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)
    np.testing.assert_array_equal(pa.intr, pb.intr)


def test_schur_tiles_match_pair_tables(pkg, gpu, shapes, monkeypatch):
    runs = _knob_runs(pkg, shapes, "a", monkeypatch, "DAB_SCHUR_TILES", ("1", "0", "1"))
    assert runs[0][0]["schur_assembly"] != runs[1][0]["schur_assembly"]
    _same_path(runs[0], runs[1])
    _bitwise(runs[0], runs[2])


def test_pair_eval_matches_camera_major(pkg, gpu, shapes, monkeypatch):
    runs = _knob_runs(pkg, shapes, "a", monkeypatch, "DAB_PAIR_EVAL", ("1", "0", "1"))
    _same_path(runs[0], runs[1])
    _bitwise(runs[0], runs[2])


def test_fused_eval_matches_two_kernel(pkg, gpu, shapes, monkeypatch):
    runs = _knob_runs(pkg, shapes, "b", monkeypatch, "DAB_EVAL_FUSED", ("1", "0", "1"))
    _same_path(runs[0], runs[1])
    _bitwise(runs[0], runs[2])


@pytest.mark.parametrize("shape", ["a", "b"])
def test_border_in_lds_rows_matches_global_sums(pkg, gpu, shapes, shape, monkeypatch):
    """k_intr_border_lds (the small camera sets' path) against k_intr_border_g (what large camera
    sets take), which DAB_INTR_BORDER_LDS=0 forces."""
    runs = _knob_runs(pkg, shapes, shape, monkeypatch, "DAB_INTR_BORDER_LDS", ("1", "0", "0"))
    _same_path(runs[0], runs[1])
    _bitwise(runs[1], runs[2])


# ---- 6. empty free set ----------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["a", "b"])
def test_empty_free_set_is_the_parent_path_bitwise(pkg, gpu, shapes, shape):
    start = shapes[shape]
    plain = start.copy()
    s = pkg.Solver(0)
    try:
        s.set_problem(plain)
        first = s.solve(_opts(pkg, 8))
    finally:
        s.close()
    runs = []
    # set then cleared; groups that select no active scalar (DISTORTION on the nk = 0 intrinsic of
    # shape a; nothing on shape b); a mask under freeze_camera is covered in test_refusals
    none_active = np.array([0, 0, 4]) if shape == "a" else np.zeros(12, np.int64)
    for how in ("cleared", "inactive"):
        p = start.copy()
        s = pkg.Solver(0)
        try:
            s.set_problem(p)
            if how == "cleared":
                s.set_intrinsics_free(7)
                assert s.get_intrinsics_free()[1] == (3 if shape == "a" else 12)
                s.set_intrinsics_free(None)
            else:
                s.set_intrinsics_free(none_active)
            assert s.get_intrinsics_free()[1:] == (0, 0)
            runs.append((s.solve(_opts(pkg, 8)), p))
            assert s.intrinsic_blocks().shape == (0, 27)
        finally:
            s.close()
    for r, p in runs:
        assert costs(r) == costs(first) and records(r) == records(first)
        assert r["num_parameters"] == first["num_parameters"]
        np.testing.assert_array_equal(p.points, plain.points)
        np.testing.assert_array_equal(p.ext, plain.ext)
        np.testing.assert_array_equal(p.intr, start.intr)


# ---- 7. refusals ----------------------------------------------------------------------------
def test_refusals(pkg, orc, gpu, shapes):
    lib = pkg.load_library()
    start = shapes["a"]
    prob = start.copy()
    s = pkg.Solver(0)
    try:
        # before dab_set_problem
        g3 = (C.c_uint8 * 3)(7, 7, 7)
        d = (C.c_double * 18)()
        n = C.c_int32()
        assert lib.dab_set_intrinsics_free(s.h, g3) == -4  # DAB_E_STATE
        assert lib.dab_get_intrinsics(s.h, d) == -4
        assert lib.dab_update_intrinsics(s.h, d) == -4
        assert lib.dab_get_intrinsic_blocks(s.h, C.byref(n), None) == -4
        s.set_problem(prob)
        plain = s.solve(_opts(pkg, 6))
        p_plain, e_plain = prob.points.copy(), prob.ext.copy()
        # group bits above 7: refused, the mask unchanged
        s.set_intrinsics_free(np.array([1, 2, 4]))
        bad = (C.c_uint8 * 3)(7, 8, 7)
        assert lib.dab_set_intrinsics_free(s.h, bad) == pkg.DAB_E_INVALID
        assert list(s.get_intrinsics_free()[0]) == [1, 2, 4]
        assert lib.dab_get_intrinsics(s.h, None) == pkg.DAB_E_INVALID
        s.set_intrinsics_free(7)
        summ = pkg._abi.DabSummary()
        # PCG, requested
        o = pkg.options(max_num_iterations=6, linear_solver_type=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG)
        s.update_parameters(start.points, start.ext)
        assert lib.dab_solve(s.h, C.byref(o), C.byref(summ)) == pkg.DAB_E_UNSUPPORTED
        assert "exact step" in pkg.last_error()
        # covariance
        assert lib.dab_covariance(s.h, None, None, None, None, C.byref(pkg.DabCovarianceInfo())) == pkg.DAB_E_UNSUPPORTED
        # nothing moved, and with the mask cleared the handle walks the parent's trajectory
        np.testing.assert_array_equal(s.get_intrinsics(), start.intr)
        s.set_intrinsics_free(None)
        again = s.solve(_opts(pkg, 6))
        assert costs(again) == costs(plain) and records(again) == records(plain)
        np.testing.assert_array_equal(prob.points, p_plain)
        np.testing.assert_array_equal(prob.ext, e_plain)
    finally:
        s.close()


def test_refusal_more_than_16_free_intrinsics(pkg, gpu):
    lib = pkg.load_library()
    prob = pkg.synth(kind=0, num_cameras=24, num_points=300, obs_per_point=6, seed=11)
    start = prob.copy()
    assert prob.intr.shape[0] == 24
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        plain = s.solve(_opts(pkg, 5))
        pts = prob.points.copy()
        s.set_intrinsics_free(7)
        assert s.get_intrinsics_free()[1] == 24
        summ = pkg._abi.DabSummary()
        o = _opts(pkg, 5)
        s.update_parameters(start.points, start.ext)
        assert lib.dab_solve(s.h, C.byref(o), C.byref(summ)) == pkg.DAB_E_UNSUPPORTED
        assert "16" in pkg.last_error()
        # sixteen of them: accepted
        g = np.zeros(24, np.int64)
        g[:16] = 2
        s.set_intrinsics_free(g)
        ok = s.solve(_opts(pkg, 5))
        assert ok["num_parameters"] == plain["num_parameters"] + 16 and ok["final_cost"] < ok["initial_cost"]
        s.update_intrinsics(start.intr)
        s.set_intrinsics_free(None)
        s.update_parameters(start.points, start.ext)
        again = s.solve(_opts(pkg, 5))
        assert costs(again) == costs(plain)
        np.testing.assert_array_equal(prob.points, pts)
    finally:
        s.close()


def test_refusal_no_free_extrinsic_and_freeze_camera(pkg, gpu, shapes):
    lib = pkg.load_library()
    start = shapes["b"]
    prob = start.copy()
    prob.ext_const = np.ones(prob.ext.shape[0], np.uint8)
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        s.set_intrinsics_free(7)
        summ = pkg._abi.DabSummary()
        o = _opts(pkg, 5)
        assert lib.dab_solve(s.h, C.byref(o), C.byref(summ)) == pkg.DAB_E_UNSUPPORTED
        assert "free extrinsic" in pkg.last_error()
        s.set_intrinsics_free(None)
        assert s.solve(_opts(pkg, 5))["num_free_ext"] == 0  # still usable
    finally:
        s.close()
    # freeze_camera: the mask is ignored, the freeze path bitwise
    runs = []
    for groups in (None, 7):
        p = start.copy()
        p.freeze_camera = True
        s = pkg.Solver(0)
        try:
            s.set_problem(p)
            if groups is not None:
                s.set_intrinsics_free(groups)
                assert s.get_intrinsics_free()[1:] == (0, 0)
            runs.append((s.solve(_opts(pkg, 6)), p))
        finally:
            s.close()
    assert costs(runs[0][0]) == costs(runs[1][0]) and records(runs[0][0]) == records(runs[1][0])
    assert runs[0][0]["num_parameters"] == runs[1][0]["num_parameters"]
    np.testing.assert_array_equal(runs[0][1].points, runs[1][1].points)
    np.testing.assert_array_equal(runs[1][1].intr, start.intr)


def test_core_solve_takes_free_intrinsics(pkg, gpu, shapes):
    a, b = shapes["a"].copy(), shapes["a"].copy()
    ra = pkg.solve(a, max_iteration=10, free_intrinsics=7)
    rb = gpu_solve(pkg, b, 7, iters=10)
    assert costs(ra) == costs(rb)
    np.testing.assert_array_equal(a.intr, b.intr)
    assert np.abs(a.intr - shapes["a"].intr).max() > 1.0


# ---- 8. two ranks ---------------------------------------------------------------------------
def test_two_ranks_match_single_handle_with_free_intrinsics(gpu):
    import os
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
           "--free-intrinsics", "7", "--iters", "6", "--solvers", "explicit"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]
    assert '"rig_0"' in p.stdout  # the rig shape ran


def test_auto_that_picks_pcg_refuses_free_intrinsics_on_every_rank(gpu):
    """The refusal for IMPLICIT_SCHUR_PCG chosen by AUTO: AUTO resolves to PCG only on several
    ranks and for a camera system that is not a small one, so two ranks on a 16 x 120 rig (135
    extrinsics, 16 intrinsics): DAB_E_UNSUPPORTED on every rank, nothing moved, and with the
    mask cleared the same handles solve (with PCG)."""
    import os
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
           "--free-intrinsics", "7", "--expect-auto-refused"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK auto refused: 2/2 ranks, 16 free intrinsics, 135 extrinsics" in p.stdout, p.stdout[-3000:]


# ---- 9. host API ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rig", "bal"])
def test_dam_set_intrinsics_free_matches_solver(pkg, gpu, kind, tmp_path):
    import importlib
    import os

    import deeparc_ref
    from golden_util import GOLDEN
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_%s.deeparc" % kind)
    groups = 7 if kind == "rig" else 2  # tiny_bal: per-camera intrinsics, the focal lengths only
    m = host.DeepArcManager()
    m.read(path)
    _, k0 = m.cameras()
    m.set_intrinsics_free(groups)
    g = host.solve(m, max_iteration=20)
    prob = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    start = prob.copy()
    d = gpu_solve(pkg, prob, groups, iters=20)
    assert g["initial_cost"] == pytest.approx(d["initial_cost"], rel=1e-12)
    assert g["final_cost"] == pytest.approx(d["final_cost"], rel=1e-12)
    assert g["num_parameters"] == d["num_parameters"]
    assert np.abs(prob.intr - start.intr).max() > 0.0
    _, k1 = m.cameras()
    used = ir.struct_mask(prob)
    np.testing.assert_array_equal(k1[used], prob.intr[used])  # the refined doubles, untruncated
    assert np.abs(k1 - k0).max() > 0.0
    # a second solve of the unchanged structure starts from the refined values
    again = host.solve(m, max_iteration=1)
    assert again["initial_cost"] == pytest.approx(g["final_cost"], rel=1e-9)
    _, k2 = m.cameras()
    out = str(tmp_path / "refined.deeparc")
    m.write(out)
    back = deeparc_ref.read_deeparc(out)["intr"]
    for i, k in enumerate(back):  # the writer prints 6 decimals; the reader truncates the centre (Q1)
        assert k["center"] == [float(int(k2[i, 0])), float(int(k2[i, 1]))]
        np.testing.assert_allclose(k["f"], k2[i, 2:2 + len(k["f"])], rtol=0, atol=0.5000001e-6)
        np.testing.assert_allclose(k["k"], k2[i, 4:4 + len(k["k"])], rtol=0, atol=0.5000001e-6)
    with pytest.raises(RuntimeError):
        m.set_intrinsics_free(8)
