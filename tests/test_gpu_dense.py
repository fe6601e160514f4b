"""The device dense Cholesky (reduced camera system of the DENSE_SCHUR-equivalent solver)
against numpy/LAPACK on random SPD systems. Tolerance: relative residual and relative
error vs numpy.linalg.solve <= 1e-12 * cond-scaled bound (well-conditioned inputs).

Below those two: the factorisation on its own — every schedule at the block edges, hard
systems, back-substitution ownership, the not-positive-definite flag and one handle over many
calls — held to K times LAPACK's own scaled backward error on the same system
(tests/dense_ref.py)."""
import numpy as np
import pytest

import dense_ref as dr

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("n", [1, 6, 63, 64, 65, 127, 128, 130, 191, 192, 193, 256, 257, 384, 449, 1000, 2048, 2050, 3001])
def test_dense_spd_solve_matches_numpy(pkg, gpu, n):
    check_solve(pkg, n)


def check_solve(pkg, n):
    rng = np.random.default_rng(n)
    M = rng.standard_normal((n, n))
    A = M @ M.T + n * np.eye(n)
    b = rng.standard_normal(n)
    s = pkg.Solver(0)
    try:
        x, ms, ok = s.dense_spd_solve(np.tril(A) + np.triu(rng.standard_normal((n, n)), 1), b)
    finally:
        s.close()
    assert ok
    ref = np.linalg.solve(A, b)
    assert np.linalg.norm(x - ref) <= 1e-12 * np.linalg.cond(A) * np.linalg.norm(ref)
    assert np.linalg.norm(A @ x - b) <= 1e-12 * np.linalg.norm(A) * np.linalg.norm(x)


def test_dense_spd_solve_detects_indefinite(pkg, gpu):
    n = 100
    A = np.eye(n)
    A[57, 57] = -1.0
    s = pkg.Solver(0)
    try:
        _, _, ok = s.dense_spd_solve(A, np.ones(n))
    finally:
        s.close()
    assert not ok


# ---- direct tests of the factorisation: schedules, block edges, hard systems -------------------
# Families, metrics, the case lists and the measured ratios behind K: tests/dense_ref.py (pinned
# under LAPACK by tests/test_dense_ref.py). Every input has its strict upper triangle NaN.
# Pass rule of a positive definite case: ok, and eta_dev <= K max(eta_ref, eps) with eta_ref
# LAPACK's scaled backward error on the same system (blockdiag: the per-block forward error
# phi likewise).
CHOL_KNOBS = ("DAB_CHOL_V1", "DAB_CHOL_STRIP", "DAB_CHOL_GROUP", "DAB_CHOL_BACK_FLOW", "DAB_CHOL_BACK_GROUPS",
              "DAB_CHOL_PREFACTOR", "DAB_CHOL_FUSE_PANEL", "DAB_CHOL_NOGRAPH", "DAB_CHOL_GRAPH_MIN",
              "DAB_CHOL_SERIAL")


def set_knobs(monkeypatch, knobs):
    """The schedule knobs are read when a handle is created: set them before Solver()."""
    for k in CHOL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for kv in filter(None, knobs.split(",")):
        name, val = kv.split("=")
        monkeypatch.setenv(name, val)


def fresh_solve(pkg, A_in, b):
    s = pkg.Solver(0)
    try:
        x, _, ok = s.dense_spd_solve(A_in, b)
    finally:
        s.close()
    return x, ok


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def check_pd(ref, x, ok, label, eta_ref=None):
    """The pass rule; prints the ratios before asserting (pytest -s shows them)."""
    eta_ref = ref["eta_ref"] if eta_ref is None else eta_ref
    eta_dev = dr.eta(ref["A"], x, ref["b"])
    ratio = eta_dev / max(eta_ref, dr.EPS)
    line = f"DENSE {label}: eta_dev/eps {eta_dev / dr.EPS:.3f} eta_ref/eps {eta_ref / dr.EPS:.3f} ratio {ratio:.3f}"
    pratio = None
    if ref.get("phi_ref") is not None:
        phi_dev = dr.phi_blocks(ref["A"], x, ref["x_true"])
        pratio = phi_dev / max(ref["phi_ref"], dr.EPS)
        line += f" phi_dev/eps {phi_dev / dr.EPS:.3f} phi_ref/eps {ref['phi_ref'] / dr.EPS:.3f} phi_ratio {pratio:.3f}"
    print(line)
    assert ok, label
    assert ratio <= dr.K, line
    assert pratio is None or pratio <= dr.K, line


@pytest.fixture(scope="module")
def inputs():
    """(lower triangle with NaN above, b) of a reference system, built once per system."""
    cache = {}

    def get(name, n, seed=0):
        key = (name, n, seed)
        if key not in cache:
            ref = dr.reference(name, n, seed)
            cache[key] = (ref, dr.lower_nan(ref["A"]))
        return cache[key]
    return get


# a. every schedule at every block edge: one 16-block, 16 +- 1, one block, one block + 1, a short
# last block with kb not a multiple of 16 (130, 200, 449, 780, 1100), the leading-dimension bump
# (511, 1023), the captured graph (1023, 1100 by default; everything with GRAPH_MIN=1)
@pytest.mark.parametrize("family", dr.EDGE_FAMILIES)
@pytest.mark.parametrize("knobs", dr.SCHEDULES, ids=[k.replace("DAB_CHOL_", "") or "default" for k in dr.SCHEDULES])
def test_schedules_at_block_edges(pkg, gpu, monkeypatch, inputs, knobs, family):
    set_knobs(monkeypatch, knobs)
    for n in dr.EDGE_SIZES:
        ref, A_in = inputs(family, n)
        x, ok = fresh_solve(pkg, A_in, ref["b"])
        check_pd(ref, x, ok, f"a {family} n={n} [{knobs or 'default'}]")


# b. ill-conditioned spectrum, exact zero tiles over 12 decades of scale, low rank + diagonal
@pytest.mark.parametrize("n", dr.HARD_SIZES)
@pytest.mark.parametrize("family", dr.HARD_FAMILIES)
def test_hard_systems(pkg, gpu, monkeypatch, inputs, family, n):
    set_knobs(monkeypatch, "")
    ref, A_in = inputs(family, n)
    x, ok = fresh_solve(pkg, A_in, ref["b"])
    check_pd(ref, x, ok, f"b {family} n={n}")


# c. back substitution ownership. In k_trsv_back_flow every z_s takes its updates L_bs^T y_b in
# the order b = last .. s + 1 whoever owns s, each update the same four-part fma sum, and y_s
# comes from the same L_ss^-1 table: ownership moves work between work-groups and changes no
# sum, so x is bitwise the default schedule's. (The grid-barrier fallback sums in another order.)
@pytest.mark.parametrize("groups,n,flow", dr.OWNERSHIP)
def test_back_substitution_ownership(pkg, gpu, monkeypatch, inputs, groups, n, flow):
    ref, A_in = inputs("wishart", n)
    set_knobs(monkeypatch, f"DAB_CHOL_BACK_GROUPS={groups}")
    x, ok = fresh_solve(pkg, A_in, ref["b"])
    check_pd(ref, x, ok, f"c wishart n={n} [BACK_GROUPS={groups}, {'flow' if flow else 'fallback'}]")
    if flow:
        set_knobs(monkeypatch, "")
        x0, ok0 = fresh_solve(pkg, A_in, ref["b"])
        assert ok0 and np.array_equal(bits(x), bits(x0))


def test_back_substitution_two_blocks_per_owner_on_the_real_grid(pkg, gpu, monkeypatch):
    """n = 8256 is 129 blocks: on the real grid of 128 work-groups, work-group 0 owns two. No
    LAPACK reference at this size (seconds); the bound is K eps, since eta_ref <= eps on lowrank
    at every size of test_dense_ref.py."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if cus // 2 != 128:
        pytest.skip(f"{cus} CUs give {cus // 2} back-substitution work-groups, not the 128 this case is about")
    set_knobs(monkeypatch, "")
    n = dr.BIG_N
    A, b, x_true = dr.system("lowrank", n)
    A_in = dr.lower_nan(A)
    x, ok = fresh_solve(pkg, A_in, b)
    del A_in
    check_pd({"A": A, "b": b}, x, ok, f"c lowrank n={n} [129 blocks on 128 work-groups]", eta_ref=dr.EPS)


# d. not positive definite: rc 1 ("not ok") and no error; x is unspecified. No wait in the
# factorisation or the back substitution depends on a matrix value: the column update polls a
# ready word and the dataflow polls y for the pending pattern, which no arithmetic produces
# (computed NaNs are quiet), and both spins are bounded.
@pytest.mark.parametrize("knobs", ["", "DAB_CHOL_PREFACTOR=0"], ids=["default", "PREFACTOR=0"])
@pytest.mark.parametrize("n,j", dr.NONPD)
def test_not_positive_definite_at_pivot(pkg, gpu, monkeypatch, inputs, n, j, knobs):
    """Pivot j turns negative only through the updates of the columns before it: in block 0
    (k_panel's own factor), at 16-block edges, in later blocks (the column update's factor),
    in the short last block, and at n = 1100 on the captured graph."""
    set_knobs(monkeypatch, knobs)
    ref, _ = inputs("wishart", n)
    B = dr.lower_nan(dr.nonpd(ref["A"], j))
    x, ok = fresh_solve(pkg, B, ref["b"])
    assert not ok


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("n", dr.NONFINITE_SIZES)
def test_not_finite_diagonal(pkg, gpu, monkeypatch, inputs, n, value):
    set_knobs(monkeypatch, "")
    ref, A_in = inputs("wishart", n)
    B = A_in.copy()
    B[n // 2, n // 2] = value
    x, ok = fresh_solve(pkg, B, ref["b"])
    assert not ok


# e. one handle, many calls: the graph cache key, the ready words, y's pending fill and the
# growth of the block scratch across consecutive solves of different n
def test_one_handle_many_calls(pkg, gpu, monkeypatch, inputs):
    set_knobs(monkeypatch, "")
    calls = []
    for n, seed in dr.SEQUENCE:
        ref, A_in = inputs("wishart", n, seed)
        calls.append((f"n={n} seed={seed}", ref, A_in, True))
    n, j = dr.SEQUENCE_NONPD
    ref, A_in = inputs("wishart", n)
    calls.append((f"nonpd n={n} j={j}", ref, dr.lower_nan(dr.nonpd(ref["A"], j)), False))
    calls.append((f"n={n} after a flagged solve", ref, A_in, True))
    s = pkg.Solver(0)
    try:
        got = [s.dense_spd_solve(A_in, ref["b"]) for _, ref, A_in, _ in calls]
    finally:
        s.close()
    for (label, ref, A_in, pd), (x, _, ok) in zip(calls, got):
        x0, ok0 = fresh_solve(pkg, A_in, ref["b"])
        assert ok == ok0 == pd, label
        assert np.array_equal(bits(x), bits(x0)), label
        if pd:
            check_pd(ref, x, ok, f"e {label}")


def test_dense_solve_between_graph_replays(pkg, gpu, monkeypatch, inputs):
    """A dense solve of the same n between two LM solves that replay the captured graph of the
    exact step (n = 170 x 6 = 1020, 16 blocks): the second trajectory is bitwise the first and
    the dense result bitwise a fresh handle's."""
    set_knobs(monkeypatch, "")
    start = pkg.synth(kind=0, num_cameras=171, num_points=4000, obs_per_point=8)
    prob = start.copy()
    opts = pkg.options(max_num_iterations=4, linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)
    n = dr.INTERLEAVED_N
    ref, A_in = inputs("wishart", n)
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        first = s.solve(opts)
        assert first["num_iterations"] >= 2
        p1, e1 = prob.points.copy(), prob.ext.copy()
        x, _, ok = s.dense_spd_solve(A_in, ref["b"])
        s.update_parameters(start.points, start.ext)
        second = s.solve(opts)
    finally:
        s.close()
    assert [it["cost"] for it in first["iterations"]] == [it["cost"] for it in second["iterations"]]
    assert first["final_cost"] == second["final_cost"] and first["termination"] == second["termination"]
    np.testing.assert_array_equal(prob.points, p1)
    np.testing.assert_array_equal(prob.ext, e1)
    x0, ok0 = fresh_solve(pkg, A_in, ref["b"])
    assert ok and ok0 and np.array_equal(bits(x), bits(x0))
    check_pd(ref, x, ok, f"e interleaved n={n}")
