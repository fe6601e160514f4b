"""Pins the CG trace of tests/step_ref.py (System.cg_trace, the reference of
tests/test_gpu_pcg_trace.py) on the CPU and proves the conditions its GPU cases rely on:

  the trace is the oracle's CG: oracle/dab_oracle.c's cg_solve run at min = max = k iterations stops
      at k with the step of cg_trace's row k (an independent float64 implementation of the same
      recurrences: it meets the GPU tests' own rule with the largest constant K_TRACE may take)
  the yardstick exists: s_k, the float64 trace against the long-double one, is at most 1e-9 at
      every (system, k) the GPU tests use, so max(s_k, c_k, eps) bounds something
  every truncated step is accepted (relative_decrease > min_relative_decrease), k = 0 included:
      the device's step can be read back as accepted parameters - initial ones
  every stop-rule case is unambiguous (step_ref.STOP_CASES)
  the schedules' preconditions that depend only on the problem
  cg() is the trace with the stop rule
"""
import numpy as np
import pytest

import lm_ref as lr
import step_ref as sr

LD = np.longdouble
KS = (0,) + sr.TRACE_KS
KMAX = max(KS)


def S_of(pkg, orc, name):
    return sr.system(pkg, orc, next(c for c in sr.TRACE_CASES if c.problem == name))


def ks_of(name):
    """Every iteration whose step a GPU test of `name` judges."""
    return sorted(set(KS) | {n for p, _, _, n, _ in sr.STOP_CASES if p == name})


def variants(name):
    return (False, True) if any(sr.y32(c) for c in sr.TRACE_CASES if c.problem == name) else (False,)


def test_the_table_names_every_problem():
    assert {c.problem for c in sr.TRACE_CASES} == set(sr.TRACE_PROBLEMS)
    assert {p for p, *_ in sr.STOP_CASES} == set(sr.TRACE_PROBLEMS)


@pytest.mark.parametrize("name", sr.TRACE_PROBLEMS)
def test_trace_is_the_oracles_cg(pkg, orc, name):
    case = next(c for c in sr.TRACE_CASES if c.problem == name and not c.opts)
    S = S_of(pkg, orc, name)
    start = sr.problem(pkg, orc, name)[0]
    _, d64, _ = S.cg_trace(KMAX)
    _, dld, _ = S.cg_trace(KMAX, LD)
    worst = 0.0
    for k in KS:
        p = start.copy()
        o = orc.solve(pkg, p, case.options(pkg, eta=1e-14, max_linear_solver_iterations=k,
                                           min_linear_solver_iterations=k))
        it = o["iterations"][1]
        assert it["success"] and it["linear_solver_iterations"] == k
        ref = max(S.step_err(d64[k], dld[k]), S.step_err(S.channel(dld[k]), dld[k]), sr.EPS)
        e = S.step_err(S.observed(p), S.channel(dld[k]))
        e64 = S.step_err(S.observed(p), S.channel(d64[k]))
        print(f"{name} k {k}: oracle against the long-double trace {e / sr.EPS:.3g} eps "
              f"({e / ref:.3g} of the yardstick), against the float64 trace {e64 / sr.EPS:.3g} eps")
        worst = max(worst, e / ref)
        assert e <= 64 * ref
    print(name, "worst ratio", worst)


@pytest.mark.parametrize("name", sr.TRACE_PROBLEMS)
def test_yardstick_exists_and_steps_are_accepted(pkg, orc, name):
    S = S_of(pkg, orc, name)
    min_rd = pkg.options().min_relative_decrease
    ks = ks_of(name)
    for y32 in variants(name):
        _, d64, _ = S.cg_trace(max(ks), np.float64, y32)
        _, dld, _ = S.cg_trace(max(ks), LD, y32)
        for k in ks:
            s = S.step_err(d64[k], dld[k])
            c = S.step_err(S.channel(dld[k]), dld[k])
            rd = S.relative_decrease(dld[k].astype(np.float64))
            print(f"{name} y32 {y32} k {k}: s_k {s / sr.EPS:.4g} eps, c_k {c / sr.EPS:.4g} eps, relative decrease {rd:.6f}")
            assert s <= 1e-9
            assert rd > min_rd


@pytest.mark.parametrize("case", sr.STOP_CASES, ids=lambda c: f"{c[0]}-eta{c[1]:g}-min{c[2]}-n{c[3]}")
def test_stop_case_is_unambiguous(pkg, orc, case):
    name, eta, min_it, n, margin = case
    S = S_of(pkg, orc, name)
    for y32 in variants(name):
        for dtype in (np.float64, LD):
            zeta = S.cg_trace(max(ks_of(name)), dtype, y32)[2]
            assert n >= max(min_it, 1) and zeta[n] <= eta / margin, (n, float(zeta[n]))
            early = zeta[max(min_it, 1):n]
            assert (early >= margin * eta).all(), early.astype(float)
        delta, its = S.cg(eta=eta, max_it=1000, min_it=min_it, y32=y32)
        assert its == n
        np.testing.assert_array_equal(delta, S.cg_trace(max(ks_of(name)), np.float64, y32)[1][n])


@pytest.mark.parametrize("name", sr.TRACE_PROBLEMS)
def test_cg_is_the_trace_with_the_stop_rule(pkg, orc, name):
    S = S_of(pkg, orc, name)
    delta, its = S.cg(eta=1e-14, max_it=1000)
    _, d, zeta = S.cg_trace(its)
    assert (zeta[1:its] >= 1e-14).all() and zeta[its] < 1e-14
    np.testing.assert_array_equal(delta, d[its])
    # the limits: max_it cuts the trace, and 0 iterations leave the cameras where they are
    for k in (0, 1, 10):
        dk, n = S.cg(eta=1e-14, max_it=k)
        assert n == k
        np.testing.assert_array_equal(dk, d[k])
    assert not d[0][S.P:].any() and d[0][:S.P].any()


def test_schedule_preconditions(pkg, orc):
    nc = {name: S_of(pkg, orc, name).L.nc for name in sr.TRACE_PROBLEMS}
    print(nc)
    # k_cg_p runs (p = z + beta p is not folded into k_cg_xr) and the product is not the fused one
    assert 6 * nc["bal344"] > 2048 and nc["bal344"] > sr.MF_CAMS_MAX
    # bal161: not fused, p folded
    assert 6 * nc["bal161"] <= 2048 and nc["bal161"] > sr.MF_CAMS_MAX
    assert nc["bal_small"] <= sr.MF_CAMS_MAX and nc["rig_small"] <= sr.MF_CAMS_MAX
    # DAB_CHUNK=64 cuts some camera's records into more than one chunk (launch_seg_final runs)
    L = S_of(pkg, orc, "bal_small").L
    cols = L.col[:, [3, 9]]
    seen = cols[(cols >= 0) & (L.col[:, :1] >= 0)]
    per_cam = np.bincount((seen - 3 * L.np) // 6, minlength=L.nc)
    print("records per camera", per_cam)
    assert per_cam.max() > 64
    # the chunked cases name the knob the tests clear
    assert all(k in sr.KNOBS for c in sr.TRACE_CASES for k in c.env)
    # rig_small has cross blocks (two extrinsics per observation), bal_small none
    assert (lr.Layout(sr.problem(pkg, orc, "rig_small")[0]).col[:, 9] >= 0).any()
    assert not (lr.Layout(sr.problem(pkg, orc, "bal_small")[0]).col[:, 9] >= 0).any()
