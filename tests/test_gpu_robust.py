"""Robust losses (dab_set_loss: Huber, soft-L1, Cauchy) through every schedule of the LM path,
on the GPU. The reference is tests/robust_ref.py (pinned by tests/test_robust_ref.py: the loss
table by finite differences, its LM loop by the oracle at the TRIVIAL loss).

Tolerances, all from the project's own bounds between two fp64 evaluations that differ in
summation order and in how the camera tables are built: blocks 1e-9 of each array's largest
entry (test_bench_blocks_match_jacobian_kernel), cost sums 1e-12, per-iteration LM cost 1e-9
relative and parameters 1e-7 against the reference and between GPU paths.

Shapes (robust_ref.bal_small / rig_small): 12 cameras x 200 points with ragged tracks of 1-8
observations (4 SELL slices, the last partial; padding slots; single-observation points) and a
3 x 5 rig with 200 points; 5 % of the observations displaced by 30-60 px, one residual exactly
0 and one within 1e-9 of Huber(1.0)'s switch s = b."""
import ctypes as C
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import lm_ref as lr
import robust_ref as rr
from golden_util import GOLDEN

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOSSES = {"huber": (rr.HUBER, 1.0), "soft_l1": (rr.SOFT_L1, 1.0), "cauchy": (rr.CAUCHY, 0.5)}
CAUCHY = ("cauchy", 0.5)


@pytest.fixture(scope="module")
def shapes(pkg, orc):
    """The two small contaminated problems (never modified: tests copy them)."""
    return {"bal": rr.bal_small(pkg, orc), "rig": rr.rig_small(pkg, orc)}


_ref_cache = {}


def reference(pkg, orc, shapes, shape, loss, freeze=False, iters=15):
    """lm_ref.lm on a copy of the shape, computed once per case."""
    key = (shape, loss, freeze, iters)
    if key not in _ref_cache:
        p = shapes[shape][0].copy()
        p.freeze_camera = freeze
        opts = pkg.options(max_num_iterations=iters, num_threads=4,
                           linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)
        _ref_cache[key] = (lr.lm(pkg, orc, p, opts, loss=LOSSES[loss]), p)
    return _ref_cache[key]


def lst_of(pkg, solver):
    return (pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR if solver == "explicit"
            else pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG)


def gpu_solve(pkg, prob, loss=None, solver="explicit", iters=15, **kw):
    """One handle, one solve, in place on prob; loss = (name, scale) or None."""
    s = pkg.Solver(0)
    try:
        if loss is not None:
            s.set_loss(*loss)
        s.set_problem(prob)
        return s.solve(pkg.options(max_num_iterations=iters, linear_solver_type=lst_of(pkg, solver), **kw))
    finally:
        s.close()


def costs(summary):
    return [it["cost"] for it in summary["iterations"]]


def records(summary):
    return [(it["iteration"], it["success"], it["valid"]) for it in summary["iterations"]]


def cg_counts(summary):
    return [it["linear_solver_iterations"] for it in summary["iterations"]]


# ---- 4. blocks and cost ---------------------------------------------------------------------
@pytest.mark.parametrize("pair", ["1", "0"])
@pytest.mark.parametrize("fused", ["1", "0"])
@pytest.mark.parametrize("loss", sorted(LOSSES))
@pytest.mark.parametrize("shape", ["bal", "rig"])
def test_blocks_and_cost_under_loss(pkg, orc, gpu, shapes, shape, loss, fused, pair, monkeypatch):
    """One evaluation pass after set_loss: V, g, U, g_c, the cross blocks and the cost against
    host sums of the sqrt(rho')-scaled rows of dab_eval_jacobians (which stay raw), in the
    fused and the two-kernel schedule and with the pair-major pass on and off."""
    monkeypatch.setenv("DAB_EVAL_FUSED", fused)
    monkeypatch.setenv("DAB_PAIR_EVAL", pair)
    prob = shapes[shape][0].copy()
    kind, a = LOSSES[loss]
    s = pkg.Solver(0)
    try:
        s.set_loss(loss, a)
        s.set_problem(prob)
        assert s.get_loss() == (loss, a)  # survives set_problem
        s.bench_eval_pass(True, 1)
        s.sync()
        b = s.bench_blocks()
        r, J = s.jacobians()
        _, raw_cost = s.residuals()
    finally:
        s.close()
    ro, _ = orc.eval_residuals(pkg, prob)
    np.testing.assert_allclose(r, ro, rtol=0, atol=1e-12 * np.abs(ro).max())  # raw, not scaled
    assert raw_cost == pytest.approx(0.5 * (ro * ro).sum(), rel=1e-12)
    ref = rr.scaled_blocks(prob, r, J, (kind, a))

    def close(x, y):
        scale = np.abs(y).max()
        assert np.abs(x - y).max() <= 1e-9 * scale, (np.abs(x - y).max(), scale)

    assert b["cost"][0] == pytest.approx(ref["cost"], rel=1e-12)
    assert abs(ref["cost"] - raw_cost) > 0.1 * raw_cost  # the loss is active on this data
    close(b["V"], ref["V"])
    close(b["g"], ref["g"])
    assert b["ug"].shape == ref["ug"].shape
    close(b["ug"][:, :21], ref["ug"][:, :21])
    close(b["ug"][:, 21:], ref["ug"][:, 21:])
    if shape == "rig":
        assert b["ux"].shape[0] > 0
        assert abs(b["ux"].sum() - ref["cross"]) <= 1e-9 * np.abs(b["ux"]).sum()


# ---- 5. LM trajectory against lm_ref.lm --------------------------------------------------------
@pytest.mark.parametrize("freeze", [False, True])
@pytest.mark.parametrize("loss", ["huber", "cauchy"])
@pytest.mark.parametrize("shape", ["bal", "rig"])
def test_lm_trajectory_matches_reference(pkg, orc, gpu, shapes, shape, loss, freeze):
    o, pref = reference(pkg, orc, shapes, shape, loss, freeze)
    prob = shapes[shape][0].copy()
    prob.freeze_camera = freeze
    g = gpu_solve(pkg, prob, (loss, LOSSES[loss][1]))
    assert g["termination"] == o["termination"], (g["message"], o["message"])
    assert g["num_iterations"] == o["num_iterations"]
    assert records(g) == records(o)
    for x, y in zip(g["iterations"], o["iterations"]):
        assert abs(x["cost"] - y["cost"]) <= 1e-9 * abs(y["cost"]), (x, y)
    assert g["initial_cost"] == pytest.approx(o["initial_cost"], rel=1e-12)
    assert g["final_cost"] == pytest.approx(o["final_cost"], rel=1e-9)
    assert np.abs(prob.points - pref.points).max() < 1e-7
    assert np.abs(prob.ext - pref.ext).max() < 1e-7
    assert len(o["iterations"]) >= 3


# ---- 6. paths agree under Cauchy(0.5) ---------------------------------------------------------
def _knob_runs(pkg, shapes, shape, solver, monkeypatch, knob, values, iters=10):
    out = []
    for v in values:
        monkeypatch.setenv(knob, v)
        p = shapes[shape][0].copy()
        out.append((gpu_solve(pkg, p, CAUCHY, solver, iters), p))
    return out


def _same_path(a, b, tol=1e-9):
    (ra, pa), (rb, pb) = a, b
    assert records(ra) == records(rb) and ra["termination"] == rb["termination"]
    assert cg_counts(ra) == cg_counts(rb)
    np.testing.assert_allclose(costs(ra), costs(rb), rtol=tol)
    assert np.abs(pa.points - pb.points).max() < 1e-7 and np.abs(pa.ext - pb.ext).max() < 1e-7


@pytest.mark.parametrize("solver", ["explicit", "pcg"])
def test_fused_eval_matches_two_kernel_under_loss(pkg, gpu, shapes, solver, monkeypatch):
    runs = _knob_runs(pkg, shapes, "bal", solver, monkeypatch, "DAB_EVAL_FUSED", ("1", "0", "1"))
    _same_path(runs[0], runs[1])
    assert costs(runs[0][0]) == costs(runs[2][0])
    np.testing.assert_array_equal(runs[0][1].points, runs[2][1].points)  # bitwise repeatable


@pytest.mark.parametrize("solver", ["explicit", "pcg"])
def test_pair_eval_matches_camera_major_under_loss(pkg, gpu, shapes, solver, monkeypatch):
    runs = _knob_runs(pkg, shapes, "rig", solver, monkeypatch, "DAB_PAIR_EVAL", ("1", "0", "1"))
    _same_path(runs[0], runs[1])
    assert costs(runs[0][0]) == costs(runs[2][0])
    np.testing.assert_array_equal(runs[0][1].points, runs[2][1].points)
    np.testing.assert_array_equal(runs[0][1].ext, runs[2][1].ext)


def test_schur_tiles_match_pair_tables_under_loss(pkg, gpu, shapes, monkeypatch):
    runs = _knob_runs(pkg, shapes, "rig", "explicit", monkeypatch, "DAB_SCHUR_TILES", ("1", "0"))
    assert runs[0][0]["schur_assembly"] != runs[1][0]["schur_assembly"]
    _same_path(runs[0], runs[1])


@pytest.mark.parametrize("shape", ["bal", "rig"])
def test_pcg_matrix_free_matches_stored_y_under_loss(pkg, gpu, shapes, shape, monkeypatch):
    runs = _knob_runs(pkg, shapes, shape, "pcg", monkeypatch, "DAB_PCG_MF", ("1", "0"))
    assert runs[0][0]["schur_assembly"] != runs[1][0]["schur_assembly"]  # both paths ran
    _same_path(runs[0], runs[1])


@pytest.mark.parametrize("shape", ["bal", "rig"])
def test_pcg_fused_matvec_matches_two_pass_under_loss(pkg, gpu, shapes, shape, monkeypatch):
    monkeypatch.setenv("DAB_PCG_MF", "0")  # the stored-Y products
    runs = _knob_runs(pkg, shapes, shape, "pcg", monkeypatch, "DAB_PCG_FUSED", ("1", "0"))
    _same_path(runs[0], runs[1])


@pytest.mark.parametrize("shape", ["bal", "rig"])
def test_pcg_converges_to_explicit_minimum_under_loss(pkg, gpu, shapes, shape):
    """PCG run to convergence (eta = 1e-14: every linear solve iterated until the Nash-Sofer
    test cannot tell it from the exact solution) takes the exact step's LM path under the
    loss, so after the 15 iterations of this file's trajectory tests it stands at EXPLICIT's
    cost (1e-6): the matrix-free products, the Schur-Jacobi preconditioner and the back
    substitution are those of the same scaled system.
    What is NOT asserted, with the figures measured on the MI355X:
    * longer runs: Cauchy(0.5) on this data is far from convex and the LM's accept / reject
      decisions are discontinuous. Over 30 iterations bal-small still agrees (186.32085687 /
      186.32085589, 5e-9) but on rig-small the two paths take the same 22 steps and part at
      iteration 23 (EXPLICIT's step invalid, PCG's accepted): 280.3133 against 280.2519, 2.2e-4;
    * inexact steps: with the default eta = 0.1, each solver run to LM convergence
      (function_tolerance 1e-14, up to 1000 iterations) ends in another local minimum:
      EXPLICIT 185.918337 / PCG 186.025987 on bal-small, EXPLICIT 279.820101 / PCG 279.441631
      (the lower one) on rig-small."""
    pe, pp = shapes[shape][0].copy(), shapes[shape][0].copy()
    e = gpu_solve(pkg, pe, CAUCHY, "explicit", iters=15)
    p = gpu_solve(pkg, pp, CAUCHY, "pcg", iters=15, eta=1e-14, max_linear_solver_iterations=1000)
    print(shape, "explicit", e["termination"], repr(e["final_cost"]), "pcg", p["termination"], repr(p["final_cost"]),
          "cg", cg_counts(p))
    assert records(e) == records(p)
    assert max(cg_counts(p)) > 6
    assert p["final_cost"] == pytest.approx(e["final_cost"], rel=1e-6)


# ---- 7. Huber(1e30) is no loss -----------------------------------------------------------------
@pytest.mark.parametrize("solver", ["explicit", "pcg"])
@pytest.mark.parametrize("shape", ["bal", "rig"])
def test_huber_with_huge_scale_equals_no_loss(pkg, gpu, shapes, shape, solver):
    """Every s <= b = 1e60, so every weight is exactly 1 and rho = s: the Huber instantiation
    must walk the TRIVIAL trajectory (1e-12: the two may contract their FMAs differently)."""
    pa, pb = shapes[shape][0].copy(), shapes[shape][0].copy()
    a = gpu_solve(pkg, pa, None, solver, iters=10)
    b = gpu_solve(pkg, pb, ("huber", 1e30), solver, iters=10)
    assert records(a) == records(b) and cg_counts(a) == cg_counts(b)
    np.testing.assert_allclose(costs(b), costs(a), rtol=1e-12)
    assert np.abs(pa.points - pb.points).max() < 1e-7


# ---- 8. TRIVIAL restores the old path ----------------------------------------------------------
@pytest.mark.parametrize("shape", ["bal", "rig"])
def test_set_trivial_restores_null_loss_path_bitwise(pkg, gpu, shapes, shape):
    start = shapes[shape][0]
    prob = start.copy()
    opts = pkg.options(max_num_iterations=8)
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        first = s.solve(opts)
        p1, e1 = prob.points.copy(), prob.ext.copy()
        s.set_loss("cauchy", 0.5)
        s.update_parameters(start.points, start.ext)
        mid = s.solve(opts)
        s.set_loss("trivial")
        assert s.get_loss() == ("trivial", 0.0)
        s.update_parameters(start.points, start.ext)
        third = s.solve(opts)
    finally:
        s.close()
    assert mid["initial_cost"] < 0.5 * first["initial_cost"]  # the middle solve did use the loss
    assert costs(first) == costs(third) and records(first) == records(third)
    np.testing.assert_array_equal(prob.points, p1)
    np.testing.assert_array_equal(prob.ext, e1)


# ---- 9. refusals -------------------------------------------------------------------------------
def test_refusals(pkg, gpu, shapes):
    prob = shapes["rig"][0].copy()
    lib = pkg.load_library()
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        s.set_loss("cauchy", 0.5)
        for kind, scale in ((4, 1.0), (-1, 1.0), (pkg.DAB_LOSS_HUBER, 0.0), (pkg.DAB_LOSS_HUBER, -1.0),
                            (pkg.DAB_LOSS_CAUCHY, float("nan")), (pkg.DAB_LOSS_SOFT_L1, float("inf"))):
            assert lib.dab_set_loss(s.h, kind, scale) == pkg.DAB_E_INVALID, (kind, scale)
            assert s.get_loss() == ("cauchy", 0.5)
        # pcg_fp32 with a loss: refused, and the handle goes on working
        o32 = pkg.options(max_num_iterations=5, pcg_fp32=1,
                          linear_solver_type=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG)
        summ = pkg._abi.DabSummary()
        assert lib.dab_solve(s.h, C.byref(o32), C.byref(summ)) == pkg.DAB_E_UNSUPPORTED
        assert "pcg_fp32" in pkg.last_error()
        before = prob.points.copy()
        np.testing.assert_array_equal(prob.points, before)
        ok = s.solve(pkg.options(max_num_iterations=5, pcg_fp32=0,
                                 linear_solver_type=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG))
        assert ok["final_cost"] < ok["initial_cost"]
        s.set_loss("trivial", -5.0)  # the scale is ignored for TRIVIAL
        assert s.get_loss() == ("trivial", 0.0)
    finally:
        s.close()


# ---- 10. it is robust --------------------------------------------------------------------------
def test_cauchy_recovers_the_inliers(pkg, orc, gpu):
    ra, rb, rc = lr.robust_triplet(pkg, orc)
    assert ra <= rc < rb, (ra, rc, rb)  # the premise, on the reference alone

    def solve(p, loss):
        names = {rr.TRIVIAL: None, rr.CAUCHY: CAUCHY}
        gpu_solve(pkg, p, names[loss[0]], "explicit", iters=25)

    ga, gb, gc = lr.robust_triplet(pkg, orc, solve)
    assert gc == pytest.approx(rc, rel=1e-6)
    assert ga <= gc < gb, (ga, gc, gb)


# ---- 11. two ranks -----------------------------------------------------------------------------
def test_two_ranks_match_single_handle_under_loss(gpu):
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "scripts", "dist_check.py"), "--device", "0", "--host-collective",
           "--loss", "cauchy:0.5", "--iters", "6", "--solvers", "explicit,pcg"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]


# ---- 12. host API ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rig", "bal"])
def test_dam_set_loss_matches_solver_set_loss(pkg, orc, gpu, kind):
    import importlib

    import deeparc_ref
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_%s.deeparc" % kind)
    m = host.DeepArcManager()
    m.read(path)
    plain = host.solve(m, max_iteration=20)
    m2 = host.DeepArcManager()
    m2.read(path)
    m2.set_loss("cauchy", 0.5)
    g = host.solve(m2, max_iteration=20)
    prob = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    d = gpu_solve(pkg, prob, CAUCHY, "explicit", iters=20)
    assert g["final_cost"] == pytest.approx(d["final_cost"], rel=1e-12)
    assert g["initial_cost"] == pytest.approx(d["initial_cost"], rel=1e-12)
    assert g["initial_cost"] < plain["initial_cost"]  # the manager's solve did use the loss
    again = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    c = pkg.solve(again, max_iteration=20, loss=CAUCHY)  # the drop-in solve() takes the pair
    assert costs(c) == costs(d)
    with pytest.raises(RuntimeError):
        m2.set_loss(7, 1.0)
