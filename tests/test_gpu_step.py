"""One LM iteration on the GPU, its linear step judged block by block against tests/step_ref.py
(pinned by tests/test_step_ref.py, which also proves every case's conditions on the CPU).

Each case runs dab_solve with max_num_iterations = 1 and the tolerances 0 under its radius,
jacobi_scaling, diagonal clip and knobs (set before the handle is created: they are read at
dab_create), asserts the schedule it meant to hit (linear_solver_type_used, schur_assembly,
pcg_matrix_free) and then judges Delta = accepted parameters - initial ones:

  exact step  every block's eta_dev <= K max(eta_64, eps); eta_64 is the case's: the worst eta of the
              float64 reference step through the same read-back channel
  PCG         every block's eta_dev <= K_PCG max(eta_cg, eps), eta_cg of the oracle's CG step
              (under a point mask step_ref's restatement of it) through the same channel
  scalars     step_norm against |Delta| (1e-12 relative plus the channel's eps |x|), cost_change /
              relative_decrease against the long-double model cost change of Delta (1e-12 of the
              sum of its absolute terms), the iteration's cost against the long-double cost at the
              returned parameters (1e-12 relative)

Each test prints its worst eta_dev / max(eta_ref, eps) and the block, and for information the worst
block against the reference's eta of that same block.

What cannot be read back follows from the constants in step_ref.py. The tile route cuts the
tri(NC) = NC (NC + 1) / 2 blocks into ceil(tri(NC) / 1024) tiles: bal_small and rig_small 1, bal46
2 (the balance odometer runs for 2 to 6), bal111 7 and bal127 8 (it does not). Batches hold at
most 64 points or batch_cap(NC) records: bal46's 300 points make 5 batches, tracks20's first batch
ends at 59 points under the cap of 1130 records and tracks10's (two LDS buffers) under 561
(test_step_ref.py proves both). Work-groups per part: min(CUs / parts, batches / (DAB_TILE_MINB x
the most parts of a tile)), at least 1, so DAB_TILE_MINB=1 gives bal46 more groups of batches than
the default 2, and 8 gives it one. The pair route cuts a pair's records into pieces of 2560:
pair2600's single pair has two. E > 128 (rig_large) and NC > 128 take the tables from global memory.
"""
import numpy as np
import pytest

import robust_ref as rr
import step_ref as sr

pytestmark = pytest.mark.gpu

LOSS_NAME = {rr.CAUCHY: "cauchy", rr.HUBER: "huber", rr.SOFT_L1: "soft_l1"}
_refs = {}


def gpu_step(pkg, case, prob, const, groups, loss, monkeypatch):
    """(summary, pcg_matrix_free) of the case's one iteration, in place on prob."""
    for k in sr.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    s = pkg.Solver(0)
    try:
        if loss[0] != rr.TRIVIAL:
            s.set_loss(LOSS_NAME[loss[0]], loss[1])
        s.set_problem(prob)
        if np.any(groups):
            s.set_intrinsics_free(groups)
        if const is not None:
            s.set_points_constant(const)
        return s.solve(case.options(pkg)), s.pcg_matrix_free()
    finally:
        s.close()


def yardstick(pkg, orc, case):
    """[nblocks] eta of the reference step through the channel, computed once per system and solver;
    its maximum is the case's eta_64 (eta_cg)."""
    key = case.key + (case.pcg,)
    if key not in _refs:
        S = sr.system(pkg, orc, case)
        prob, const, groups, loss = sr.problem(pkg, orc, case.problem)
        if not case.pcg:
            step = S.channel(S.step64())
        elif const is None:
            p = prob.copy()
            o = orc.solve(pkg, p, case.options(pkg))
            assert o["iterations"][1]["success"]
            step = S.observed(p)
        else:
            step = S.channel(S.cg(eta=1e-14, max_it=1000)[0])
        _refs[key] = S.block_eta(step)
        _refs[key].setflags(write=False)
    return _refs[key]


@pytest.mark.parametrize("case", sr.CASES, ids=lambda c: c.id)
def test_step(pkg, orc, gpu, case, monkeypatch):
    start, const, groups, loss = sr.problem(pkg, orc, case.problem)
    S = sr.system(pkg, orc, case)
    eta_ref = yardstick(pkg, orc, case)
    prob = start.copy()
    g, mf = gpu_step(pkg, case, prob, const, groups, loss, monkeypatch)

    # the schedule the case names
    want_solver = pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG if case.pcg else pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR
    assert g["linear_solver_type_used"] == want_solver
    assert g["schur_assembly"] == case.assembly, (g["schur_assembly"], case.assembly)
    if case.pcg:
        assert mf == case.assembly
    assert g["num_parameters"] == S.n and g["num_free_ext"] == S.L.nc and g["num_free_points"] == S.L.np
    assert len(g["iterations"]) == 2, g["message"]
    it = g["iterations"][1]
    assert it["valid"] and it["success"], it
    if case.pcg:
        assert it["linear_solver_iterations"] >= 21  # both residual resets ran

    # what is constant stays, bit for bit
    free_pt = np.zeros(start.points.shape[0], bool)
    free_pt[S.L.pt_of] = True
    free_ext = np.zeros(start.ext.shape[0], bool)
    free_ext[S.L.ext_of] = True
    np.testing.assert_array_equal(prob.points[~free_pt], start.points[~free_pt])
    np.testing.assert_array_equal(prob.ext[~free_ext], start.ext[~free_ext])
    np.testing.assert_array_equal(prob.intr[~S.L.act], start.intr[~S.L.act])

    # the step, block by block, against the case's yardstick
    delta = S.observed(prob)
    eta_dev = S.block_eta(delta)
    ref = max(float(eta_ref.max()), sr.EPS)
    ratio = eta_dev / ref
    b = int(np.argmax(ratio))
    own = eta_dev / np.maximum(eta_ref, sr.EPS)  # each block against the reference's same block: printed only
    k = sr.K_PCG if case.pcg else sr.K
    # the scalars
    nrm = S.step_norm(delta)
    e_norm = abs(it["step_norm"] - nrm) / (1e-12 * nrm + sr.EPS * float(np.linalg.norm(S.x0)))
    mc, mscale = S.model_cost_change(delta)
    e_model = abs(it["cost_change"] / it["relative_decrease"] - mc) / (1e-12 * mscale)
    cost = S.cost(prob=prob)
    e_cost = abs(it["cost"] - cost) / (1e-12 * cost)
    print(f"STEP {case.id} group {case.group}{'/pcg' if case.pcg else ''} assembly {g['schur_assembly']} "
          f"cg {it['linear_solver_iterations']} worst eta_dev / max(eta_ref, eps) {ratio[b]:.3f} at {S.block_name(b)} "
          f"(eta_dev {eta_dev[b] / sr.EPS:.4g} eps, eta_ref {ref / sr.EPS:.4g} eps; against its own block "
          f"{own.max():.1f} at {S.block_name(int(np.argmax(own)))}) "
          f"scalars / bound: step_norm {e_norm:.3g} model {e_model:.3g} cost {e_cost:.3g}")
    assert ratio[b] <= k, f"{S.block_name(b)}: eta_dev {eta_dev[b]:.3g} > {k} max(eta_ref {ref:.3g}, eps)"
    assert e_norm <= 1.0 and e_model <= 1.0 and e_cost <= 1.0
    assert g["initial_cost"] == pytest.approx(S.cost0, rel=1e-12)
