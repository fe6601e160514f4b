"""The implicit-Schur PCG on the GPU, iterate by iterate, against the CG trace of tests/step_ref.py
(System.cg_trace; tests/test_pcg_trace_ref.py pins it to the oracle and proves every condition used
here on the CPU).

A converged CG forgives an operator wrong in a low-order term, a direction update off by one
iteration or a residual reset that reads a stale product. So every schedule of
step_ref.PCG_SCHEDULES (matrix-free and stored-Y products, fused or in two passes, the chunked
camera-side reduction, one or many CG work-groups with p folded or in k_cg_p, float32 Y records)
is stopped after exactly k iterations (min = max = k, eta 1e-14, one LM iteration) and its step
Delta = accepted parameters - initial ones is judged against row k of the long-double trace:

  e_k = |D (Delta_dev - channel(Delta_k^ld))|_inf / |D Delta_k^ld|_inf <= K_TRACE max(s_k, c_k, eps)

D = sqrt(diag H) in the units of Delta, s_k the float64 trace against the long-double one (what
float64 arithmetic may move iterate k), c_k what the read-back channel loses. k runs over
step_ref.TRACE_KS: 10 and 20 are the residual resets (update modes 1 and 2 and the exact product),
11 and 21 the first directions from a reset residual. float32 stored Y is judged against the trace
with Y rounded to float32; matrix-free float32 arithmetic has no such restatement and is only
checked for its counts and for reproducibility.

Also: max_linear_solver_iterations = 0 (no camera moves, the points take the step of the
back substitution alone), the stop rules at iterations known from the reference (step_ref.
STOP_CASES: eta alone, eta with min_linear_solver_iterations, on and right after a reset), and
run-to-run equality of the converged solve (eta 1e-14, 1000 iterations): four runs on three fresh
handles give the same count, bitwise equal parameters and the same cost.
"""
import numpy as np
import pytest

import step_ref as sr

pytestmark = pytest.mark.gpu

LD = np.longdouble
JUDGED = [c for c in sr.TRACE_CASES if sr.judged(c)]
KMAX = max(sr.TRACE_KS)


def group(case):
    return "y32" if sr.y32(case) else ("mf" if case.assembly == sr.MATRIX_FREE else "stored")


def set_env(case, monkeypatch):
    for k in sr.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)


def solve(pkg, case, prob, solver=None, **over):
    """The summary of the case's one LM iteration on `prob` (in place), on a fresh handle unless one
    is given; the knobs must be set already (they are read when the handle is created)."""
    s = solver or pkg.Solver(0)
    try:
        s.set_problem(prob)
        g = s.solve(case.options(pkg, **over))
        assert g["schur_assembly"] == case.assembly, (g["schur_assembly"], case.assembly)
        assert s.pcg_matrix_free() == case.assembly
        assert g["linear_solver_type_used"] == pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG
        assert len(g["iterations"]) == 2, g["message"]
        return g
    finally:
        if solver is None:
            s.close()


def traces(S, case, kmax):
    y32 = sr.y32(case)
    return S.cg_trace(kmax, np.float64, y32)[1], S.cg_trace(kmax, LD, y32)[1]


def ratio(S, case, k, start, prob, kmax=KMAX):
    """e_k / max(s_k, c_k, eps) of the solved `prob`, after the checks every truncated solve shares."""
    free_pt = np.zeros(start.points.shape[0], bool)
    free_pt[S.L.pt_of] = True
    free_ext = np.zeros(start.ext.shape[0], bool)
    free_ext[S.L.ext_of] = True
    np.testing.assert_array_equal(prob.points[~free_pt], start.points[~free_pt])
    np.testing.assert_array_equal(prob.ext[~free_ext], start.ext[~free_ext])
    np.testing.assert_array_equal(prob.intr, start.intr)
    d64, dld = traces(S, case, kmax)
    ref = max(S.step_err(d64[k], dld[k]), S.step_err(S.channel(dld[k]), dld[k]), sr.EPS)
    return S.step_err(S.observed(prob), S.channel(dld[k])) / ref


@pytest.mark.parametrize("case", JUDGED, ids=lambda c: c.id)
def test_trace(pkg, orc, gpu, case, monkeypatch):
    start = sr.problem(pkg, orc, case.problem)[0]
    S = sr.system(pkg, orc, case)
    set_env(case, monkeypatch)
    out = {}
    for k in sr.TRACE_KS:
        prob = start.copy()
        g = solve(pkg, case, prob, eta=1e-14, max_linear_solver_iterations=k, min_linear_solver_iterations=k)
        it = g["iterations"][1]
        assert it["linear_solver_iterations"] == k, (k, it)
        assert it["valid"] and it["success"], (k, it)
        out[k] = ratio(S, case, k, start, prob)
    worst = max(out, key=out.get)
    print(f"TRACE {case.id} group {group(case)} worst e_k / max(s_k, c_k, eps) {out[worst]:.3f} at k {worst}; all "
          + " ".join(f"{k}:{r:.2f}" for k, r in out.items()))
    assert out[worst] <= sr.K_TRACE, f"k {worst}: e_k is {out[worst]:.3g} of the yardstick, over {sr.K_TRACE}"


@pytest.mark.parametrize("case", JUDGED, ids=lambda c: c.id)
def test_zero_iterations(pkg, orc, gpu, case, monkeypatch):
    """max_linear_solver_iterations = 0: the CG returns x = 0 without an iteration, and the points
    take the step of the back substitution alone."""
    start = sr.problem(pkg, orc, case.problem)[0]
    S = sr.system(pkg, orc, case)
    set_env(case, monkeypatch)
    prob = start.copy()
    g = solve(pkg, case, prob, eta=1e-14, max_linear_solver_iterations=0)
    it = g["iterations"][1]
    assert it["linear_solver_iterations"] == 0
    assert it["valid"] and it["success"], it
    np.testing.assert_array_equal(prob.ext, start.ext)
    r = ratio(S, case, 0, start, prob)
    print(f"TRACE0 {case.id} group {group(case)} e_0 / max(s_0, c_0, eps) {r:.3f}")
    assert r <= sr.K_TRACE


@pytest.mark.parametrize("case", sr.TRACE_CASES, ids=lambda c: c.id)
def test_stop_rules(pkg, orc, gpu, case, monkeypatch):
    start = sr.problem(pkg, orc, case.problem)[0]
    S = sr.system(pkg, orc, case)
    set_env(case, monkeypatch)
    worst = 0.0
    for name, eta, min_it, n, _ in sr.STOP_CASES:
        if name != case.problem:
            continue
        prob = start.copy()
        g = solve(pkg, case, prob, eta=eta, max_linear_solver_iterations=1000, min_linear_solver_iterations=min_it)
        it = g["iterations"][1]
        assert it["linear_solver_iterations"] == n, (eta, min_it, n, it["linear_solver_iterations"])
        assert it["valid"] and it["success"], it
        if sr.judged(case):
            r = ratio(S, case, n, start, prob)
            print(f"STOP {case.id} group {group(case)} eta {eta:g} min {min_it} n {n} e_n / max(s_n, c_n, eps) {r:.3f}")
            worst = max(worst, r)
    assert worst <= sr.K_TRACE


@pytest.mark.parametrize("case", sr.TRACE_CASES, ids=lambda c: c.id)
def test_run_to_run_equality(pkg, orc, gpu, case, monkeypatch):
    """dab_pcg.hip: "every reduction has a fixed order, so results are bitwise reproducible". Four
    converged solves: three fresh handles, and the third once more after set_problem."""
    start = sr.problem(pkg, orc, case.problem)[0]
    S = sr.system(pkg, orc, case)
    set_env(case, monkeypatch)
    runs = []
    for i in range(3):
        s = pkg.Solver(0)
        try:
            for _ in range(2 if i == 2 else 1):
                prob = start.copy()
                g = solve(pkg, case, prob, solver=s)
                it = g["iterations"][1]
                assert it["valid"] and it["success"], it
                runs.append((it["linear_solver_iterations"], it["cost"], prob))
        finally:
            s.close()
    counts = [r[0] for r in runs]
    want = S.cg(eta=1e-14, max_it=1000, y32=sr.y32(case))[1]
    print(f"EQUAL {case.id} counts {counts} reference {want} costs {[r[1] for r in runs]}")
    assert len(runs) == 4 and len(set(counts)) == 1, counts
    for _, cost, prob in runs[1:]:
        np.testing.assert_array_equal(prob.points, runs[0][2].points)
        np.testing.assert_array_equal(prob.ext, runs[0][2].ext)
        assert cost == runs[0][1]
    # The reference's own count moves by one between its two implementations on rig_small
    # (test_step_ref.py); on the BAL shapes they agree, and the device must be within 2. Not under
    # matrix-free float32 arithmetic: zeta < 1e-14 needs Q to stop falling to 1e-14 of itself, which
    # products with 6e-8 of noise reach only where the noise lets them (40 iterations measured,
    # a residual reset, against 28), so that count says nothing about the recurrences.
    if case.problem != "rig_small" and sr.judged(case):
        assert abs(counts[0] - want) <= 2, (counts[0], want)
