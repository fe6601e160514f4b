"""Pins tests/step_ref.py (the reference of tests/test_gpu_step.py) on the CPU: the refined step
solves every case's system to eta_ref <= 0.01 eps, the float64 step is the one of the
reference LM (lm_ref.lm), and every GPU case meets the conditions it relies on (first step accepted, the
schedule facts that depend only on the problem, at least 21 CG iterations for the PCG cases).
Every case runs here, the 2600-point one included (its system takes a fraction of a second)."""
import numpy as np
import pytest

import lm_ref as lr
import step_ref as sr

UNIQUE = list({c.key: c for c in reversed(sr.CASES)}.values())[::-1]  # the first case of every system


@pytest.mark.parametrize("case", UNIQUE, ids=lambda c: c.id)
def test_refined_step_solves_the_system(pkg, orc, case):
    S = sr.system(pkg, orc, case)
    delta, eta, rounds = S.refined()
    e64 = S.block_eta(S.step64()).max()
    print(case.id, "n", S.n, "eta_ref", eta / sr.EPS, "eps after", rounds, "rounds; float64 step", e64 / sr.EPS, "eps")
    assert eta <= sr.ETA_REF_MAX
    assert S.block_eta(delta).max() == pytest.approx(eta, rel=1e-6)  # the block view loses nothing
    if case.problem != "near_min":  # there float64's own g = As^T r has lost five digits to cancellation
        assert e64 <= 16 * sr.EPS   # a backward stable float64 solve, before the channel


@pytest.mark.parametrize("jacobi", [1, 0])
def test_metric_is_invariant_under_the_scaling(pkg, orc, jacobi):
    """One Delta (the float64 step, off by 1e-6 in every component so that its residual is no
    rounding noise) judged in the case's system and in the same system under another diagonal
    scaling (powers of two: rows As t, damping d t^2, y / t): every eta_i stays."""
    prob = sr.problem(pkg, orc, "bal_small")[0]
    S = sr.System(pkg, orc, prob.copy(), 1e4, jacobi)
    rng = np.random.default_rng(3)
    delta = S.step64() * (1.0 + 1e-6 * rng.standard_normal(S.n))
    e = S.eta_rows(delta).astype(float)
    t = 2.0 ** rng.integers(-20, 21, S.n)
    T = sr.System(pkg, orc, prob.copy(), 1e4, jacobi)
    T.scale = S.scale * t
    T.vs = S.vs * np.append(t, 0.0)[S.col]
    T.d = S.d * t * t
    T._reduce()
    assert e.max() > 1e3 * sr.EPS
    np.testing.assert_allclose(T.eta_rows(delta).astype(float), e, rtol=1e-9, atol=1e-12 * e.max())


def _one_iteration(pkg, **kw):
    return pkg.options(max_num_iterations=1, function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0,
                       num_threads=4, **kw)


@pytest.mark.parametrize("name", ["bal_small", "shape_a", "third_const"])
def test_float64_step_is_the_reference_lm_step(pkg, orc, name):
    prob, const, groups, loss = sr.problem(pkg, orc, name)
    # At radius 1 the damped, Jacobi-scaled H has a condition number of some tens (1 + its largest
    # eigenvalue), so two backward stable float64 solves of it agree to about 1e-14. At the
    # default 1e4 it reaches 1e5 and they differ by their own forward errors (1.6e-12 on shape_a).
    S = sr.System(pkg, orc, prob.copy(), radius=1.0, const=const, groups=groups, loss=loss)
    p = prob.copy()
    o = _one_iteration(pkg, initial_trust_region_radius=1.0)
    s = lr.lm(pkg, orc, p, o, const=const, groups=groups, loss=loss)
    assert s["iterations"][1]["success"] and s["num_parameters"] == S.n
    got, want = S.observed(p), S.channel(S.step64())
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(name, "step", np.linalg.norm(want), "relative difference", err)
    assert err <= 1e-12
    # the scalars of that iteration, the reference LM's against the long-double ones
    it = s["iterations"][1]
    assert it["step_norm"] == pytest.approx(S.step_norm(got), rel=1e-12)
    mc, scale = S.model_cost_change(got)
    assert abs(it["cost_change"] / it["relative_decrease"] - mc) <= 1e-12 * scale
    assert it["cost"] == pytest.approx(S.cost(prob=p), rel=1e-12)
    assert s["initial_cost"] == pytest.approx(S.cost0, rel=1e-12)


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: c.id)
def test_case_conditions(pkg, orc, case):
    prob, const, groups, loss = sr.problem(pkg, orc, case.problem)
    S = sr.system(pkg, orc, case)
    o = case.options(pkg)
    # the first step is valid and accepted
    delta = S.step64()
    mc = S.model_cost_change(delta)[0]
    rd = S.relative_decrease(delta)
    print(case.id, "model cost change", mc, "relative decrease", rd)
    assert mc > 0.0 and rd > o.min_relative_decrease
    # schedule facts that depend only on the problem
    L, f = S.L, case.facts
    per_point, _ = sr.free_cameras_per_point(prob, const)
    if "nc" in f:
        assert L.nc == f["nc"]
    if "maxrec" in f:
        assert per_point.max() == f["maxrec"] and (per_point == f["maxrec"]).sum() == 1
        assert np.median(per_point) <= 4  # among ordinary points
    if case.assembly == sr.TILES and not case.pcg:
        assert 0 < L.nc <= sr.MF_CAMS_MAX and per_point.max() <= sr.TILE_MAX_REC
        assert prob.ext.shape[0] <= sr.SMALL_TABS and prob.intr.shape[0] <= sr.SMALL_TABS
    if f.get("big_tabs"):
        assert prob.ext.shape[0] > sr.SMALL_TABS
    if "chunk" in f:
        assert sr.shared_points(prob, const)[1, 0] == 2600 > sr.PAIR_CHUNK  # two pieces: 2600 <= 2 * 2560
    if "holes" in f:
        sh = sr.shared_points(prob, const)
        assert (sh[np.tril_indices(L.nc, -1)] == 0).any()
    if "cut" in f:
        single = case.env.get("DAB_TILE_SINGLE", "1") != "0"
        first = sr.first_batch_points(prob, single)
        print("first batch", first, "points, cap", sr.batch_cap(L.nc, single), "records")
        assert first < sr.BATCH_POINTS  # cut by the record cap
    if case.problem == "bal46":
        assert sr.TILE_BLOCKS < L.nc * (L.nc + 1) // 2 <= 2 * sr.TILE_BLOCKS  # two tiles
        assert L.np >= 4 * sr.BATCH_POINTS                                   # at least four batches
    if case.problem == "bal111":
        assert -(-(L.nc * (L.nc + 1) // 2) // sr.TILE_BLOCKS) == 7            # seven tiles: no odometer
    if case.clip:
        print("clipped below / above", S.clipped)
        assert S.clipped[1] > 0
        if case.facts.get("both_clips"):
            assert S.clipped[0] > 0 and S.clipped[0] + S.clipped[1] < S.n
    if case.problem == "bal_1e8":
        assert np.abs(S.r).max() > 1e7
    if case.problem == "near_min":
        g0 = np.abs(sr.system(pkg, orc, sr.CASES[0]).g / sr.system(pkg, orc, sr.CASES[0]).scale).max()
        assert np.abs(S.g / S.scale).max() < 1e-4 * g0


PCG_KEYS = list({c.key: c for c in reversed(sr.CASES) if c.pcg}.values())[::-1]


@pytest.mark.parametrize("case", PCG_KEYS, ids=lambda c: c.id)
def test_pcg_cases_run_both_residual_resets(pkg, orc, case):
    """The oracle's CG at eta = 1e-14 needs at least 21 iterations on every PCG case (the residual
    is recomputed at iterations 10 and 20); step_ref.cg restates it (the yardstick under a point
    mask, which the oracle cannot express) and is pinned to it where both run."""
    prob, const, groups, loss = sr.problem(pkg, orc, case.problem)
    S = sr.system(pkg, orc, case)
    delta, its = S.cg(eta=1e-14, max_it=1000)
    print(case.id, "cg iterations", its, "eta", S.block_eta(S.channel(delta)).max() / sr.EPS, "eps")
    assert its >= 21
    if const is None:
        p = prob.copy()
        s = orc.solve(pkg, p, case.options(pkg))
        assert s["iterations"][1]["success"]
        oits = s["iterations"][1]["linear_solver_iterations"]
        eo = S.block_eta(S.observed(p)).max()
        print("oracle's cg iterations", oits, "eta", eo / sr.EPS, "eps")
        assert oits >= 21 and abs(oits - its) <= 2
        # both stop on the same rule: their etas are of one order
        ec = S.block_eta(S.channel(delta)).max()
        assert max(eo, ec) <= 1e3 * max(min(eo, ec), sr.EPS)
