"""Gaussian priors on intrinsics on the GPU (dab_set_intr_priors) through dab_solve and
dab_covariance_intrinsics, against tests/intrprior_ref.py (pinned by tests/test_intrprior_ref.py,
which also asserts the reference's own spread on every trajectory case, at most 1e-10 of the cost
and 1e-8 of the parameters, and that every case differs from its no-prior trajectory by at least
100 tolerances).

Tolerances are the project's: same iteration records, termination and num_residuals,
initial_cost 1e-12, per-iteration cost 1e-9 relative, points and extrinsics 1e-7, intrinsics
1e-7 max(1, |v|); covariance blocks 64 kappa 2^-53 max|Sigma| (tests/test_gpu_cov_intrinsics.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_intr_ref as czr
import intr_ref as ir
import intrprior_ref as zr
import lm_ref as lr
import ptconst_ref as pr
import robust_ref as rr

pytestmark = pytest.mark.gpu

TRIVIAL = (rr.TRIVIAL, 1.0)
LOSS_NAME = {rr.TRIVIAL: None, rr.CAUCHY: "cauchy"}
SENTINEL = -12345.0625


def records(s):
    return [(i["success"], i["valid"]) for i in s["iterations"]]


def costs(s):
    return [i["cost"] for i in s["iterations"]]


def _opts(pkg, iters, **kw):
    return pkg.options(max_num_iterations=iters, num_threads=4, linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR,
                       **kw)


def gpu_solve(pkg, prob, intr_priors, groups, iters=25, ext_priors=None, point_priors=None, const=None, loss=None):
    s = pkg.Solver(0)
    try:
        if loss and loss[0] != rr.TRIVIAL:
            s.set_loss(LOSS_NAME[loss[0]], loss[1])
        s.set_problem(prob)
        if np.any(groups):
            s.set_intrinsics_free(groups)
        if const is not None:
            s.set_points_constant(const)
        if ext_priors is not None:
            s.set_ext_priors(*ext_priors)
        if point_priors is not None:
            s.set_point_priors(*point_priors)
        if intr_priors is not None:
            s.set_intr_priors(*intr_priors)
        out = s.solve(_opts(pkg, iters))
        out["num_effective"] = s.get_intr_priors()[3]
        return out
    finally:
        s.close()


_ref = {}


def traj_ref(pkg, orc, name):
    """(summary, solved problem, the case) of intrprior_ref.lm, once per case, never modified."""
    if name not in _ref:
        case = zr.make_case(pkg, orc, zr.TRAJ[name])
        start, ip, ep, pp, m, loss, groups, iters = case
        p = start.copy()
        out = zr.lm(pkg, orc, p, _opts(pkg, iters), priors=ep, point_priors=pp, intr_priors=ip, const=m, groups=groups,
                    loss=loss)
        _ref[name] = (out, p, case)
    return _ref[name]


def check_against(tag, g, prob, ref):
    o, pref, case = ref
    start, m = case[0], case[4]
    err = max((abs(x - y) / abs(y) for x, y in zip(costs(g), costs(o))), default=0.0)
    print(tag, g["termination"], g["num_iterations"], "cost", g["initial_cost"], "->", g["final_cost"], "rejected",
          g["num_unsuccessful_steps"], "assembly", g["schur_assembly"], "max rel cost err", err, "points err",
          np.abs(prob.points - pref.points).max(), "ext err", np.abs(prob.ext - pref.ext).max(), "intr err",
          (np.abs(prob.intr - pref.intr) / np.maximum(1.0, np.abs(pref.intr))).max())
    assert g["termination"] == o["termination"], (g["message"], o["message"])
    assert g["num_iterations"] == o["num_iterations"]
    assert records(g) == records(o)
    assert g["num_residuals"] == o["num_residuals"]
    assert g["initial_cost"] == pytest.approx(o["initial_cost"], rel=1e-12)
    for x, y in zip(g["iterations"], o["iterations"]):
        assert abs(x["cost"] - y["cost"]) <= 1e-9 * abs(y["cost"]), (x, y)
    assert np.abs(prob.points - pref.points).max() < 1e-7
    assert np.abs(prob.ext - pref.ext).max() < 1e-7
    assert (np.abs(prob.intr - pref.intr) <= 1e-7 * np.maximum(1.0, np.abs(pref.intr))).all()
    if m is not None:
        np.testing.assert_array_equal(prob.points[m], start.points[m])
    assert g["num_parameters"] == o["num_parameters"] and g["num_free_ext"] == o["num_free_ext"]


def run_traj(pkg, orc, name):
    ref = traj_ref(pkg, orc, name)
    start, ip, ep, pp, m, loss, groups, iters = ref[2]
    prob = start.copy()
    g = gpu_solve(pkg, prob, ip, groups, iters, ep, pp, m, loss)
    return g, prob, ref


# ---- 1. trajectories ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [t[0] for t in zr.TRAJECTORIES])
def test_trajectory_matches_reference(pkg, orc, gpu, name):
    g, prob, ref = run_traj(pkg, orc, name)
    check_against(name, g, prob, ref)
    t = zr.TRAJ[name]
    assert (g["num_iterations"], g["num_unsuccessful_steps"]) == t[-1]
    nprior = len(ref[2][1][0])
    assert g["num_effective"] == nprior
    extra = 6 * nprior + (6 * len(ref[2][2][0]) if ref[2][2] else 0) + (3 * len(ref[2][3][0]) if ref[2][3] else 0)
    assert g["num_residuals"] == 2 * prob.num_obs + extra
    assert np.abs(prob.intr - ref[2][0].intr).max() > 1e-4  # the intrinsics moved


def test_prior_counts_covered(pkg, orc):
    """1 (shape_c), 3 with mixed models and inactive slots (shape_a), 12, and 16 (the maximum)."""
    n = {name: len(zr.make_case(pkg, orc, zr.TRAJ[name])[1][0]) for name in ("C-calib", "A-calib", "B-calib",
                                                                              "pcB-first16-calib")}
    assert n == {"C-calib": 1, "A-calib": 3, "B-calib": 12, "pcB-first16-calib": 16}


@pytest.mark.parametrize("lds", ["1", "0"])
def test_trajectory_both_border_paths(pkg, orc, gpu, lds, monkeypatch):
    monkeypatch.setenv("DAB_INTR_BORDER_LDS", lds)  # read when the handle is created
    g, prob, ref = run_traj(pkg, orc, "A-calib")
    check_against(f"A-calib/lds={lds}", g, prob, ref)


@pytest.mark.parametrize("tiles", ["0", "1"])
def test_trajectory_both_assemblies(pkg, orc, gpu, tiles, monkeypatch):
    monkeypatch.setenv("DAB_SCHUR_TILES", tiles)  # read when the handle is created
    g, prob, ref = run_traj(pkg, orc, "pcR-calib-s16")
    check_against(f"pcR-calib-s16/tiles={tiles}", g, prob, ref)
    assert g["schur_assembly"] == int(tiles)
    assert g["num_unsuccessful_steps"] > 0


# ---- 2. dab_eval_intr_priors, initial_cost, the blocks --------------------------------------------
def _eval_case(pkg, orc):
    """shape_b without the observations of intrinsic 7, intrinsics 2 and 3 constant; the 9 free
    ones, 3 (constant) and 7 (unreferenced) named."""
    base = ir.shape_b(pkg, orc)
    unref, const = 7, [2, 3]
    base = base.subset(base.obs_intr != unref).copy()
    groups = np.full(base.intr.shape[0], 7)
    groups[const] = 0
    idx, mu, A = zr.calib(base, groups)
    assert len(idx) == 9 and unref not in idx and 3 not in idx
    rng = np.random.default_rng(4)
    idx = np.concatenate([[3], idx[:4], [unref], idx[4:]]).astype(np.int32)
    mu = np.concatenate([base.intr[[3]] + 1.0, mu[:4], base.intr[[unref]] - 2.0, mu[4:]])
    A = np.concatenate([np.eye(6)[None], A[:4], 30.0 * rng.standard_normal((1, 6, 6)), A[4:]])
    return base, groups, (idx, mu, A), (0, 5)


@pytest.mark.parametrize("loss", [None, pr.CAUCHY2])
def test_eval_intr_priors_and_initial_cost_against_numpy(pkg, orc, gpu, loss):
    prob, groups, ip, ignored = _eval_case(pkg, orc)
    want, want_cost = zr.intr_prior_residuals(prob, ip, groups)
    assert not want[list(ignored)].any() and np.abs(want).max() > 1.0
    # numpy on its own, not through the reference's Layout: nf = 1 drops column 3
    act = np.array([1, 1, 1, 0, 1, 1], bool)
    for j in range(len(ip[0])):
        if j not in ignored:
            np.testing.assert_allclose(want[j], ip[2][j][:, act] @ (prob.intr[ip[0][j]] - ip[1][j])[act], rtol=1e-13)
    s = pkg.Solver(0)
    try:
        if loss:
            s.set_loss(LOSS_NAME[loss[0]], loss[1])
        s.set_problem(prob)
        s.set_intr_priors(*ip)
        r0, c0 = s.eval_intr_priors()            # nothing free yet: every prior is ignored
        assert not r0.any() and c0 == 0.0 and s.get_intr_priors()[3] == 0
        s.set_intrinsics_free(groups)
        assert s.get_intr_priors()[3] == len(ip[0]) - 2
        r, cost = s.eval_intr_priors()
        print("residual err", np.abs(r - want).max(), "of", np.abs(want).max(), "cost", cost, want_cost)
        assert np.abs(r - want).max() <= 1e-12 * np.abs(want).max()
        assert not r[list(ignored)].any()
        assert cost == pytest.approx(want_cost, rel=1e-12)
        out = s.solve(_opts(pkg, 2))
        # 0.5 sum rho of the observations (never the prior under the loss) + the prior cost
        rho_cost = rr.cost(*(loss or TRIVIAL), orc.eval_residuals(pkg, _eval_case(pkg, orc)[0])[0])
        assert out["initial_cost"] == pytest.approx(rho_cost + want_cost, rel=1e-12)
        assert out["num_residuals"] == 2 * prob.num_obs + 6 * (len(ip[0]) - 2)
        # at the refined intrinsics now
        r2, cost2 = s.eval_intr_priors()
        want2, want_cost2 = zr.intr_prior_residuals(prob, ip, groups)
        assert np.abs(r2 - want2).max() <= 1e-12 * np.abs(want2).max() and cost2 == pytest.approx(want_cost2, rel=1e-12)
        assert cost2 != cost
    finally:
        s.close()


def test_intrinsic_blocks_raw_after_bench_pass_with_priors_after_solve(pkg, orc, gpu):
    prob = ir.shape_a(pkg, orc)
    ip = zr.calib(prob, 7)
    r, _ = orc.eval_jacobians(pkg, prob)
    raw = ir.scaled_intrinsic_blocks(prob, r, ir.jz(prob), 7, TRIVIAL)
    # A^T A | A^T r over the active slots, per free intrinsic
    L = lr.Layout(prob, None, 7)
    add = np.zeros_like(raw)
    iu = np.triu_indices(6)
    for j, i in enumerate(ip[0]):
        act = L.act[i]
        A = ip[2][j] * act[None, :]
        res = A @ np.where(act, prob.intr[i] - ip[1][j], 0.0)
        add[j] = np.concatenate([(A.T @ A)[iu], A.T @ res])
    assert np.abs(add).max() > 1e-3 * np.abs(raw).max()
    s = pkg.Solver(0)
    try:
        s.set_problem(prob.copy())
        s.set_intrinsics_free(7)
        s.set_intr_priors(*ip)
        s.bench_eval_pass(True, 1)
        s.sync()
        z_raw = s.intrinsic_blocks()
        s.solve(_opts(pkg, 0))
        z_solve = s.intrinsic_blocks()
        s.bench_eval_pass(True, 1)
        s.sync()
        z_again = s.intrinsic_blocks()
    finally:
        s.close()
    scale = np.abs(raw + add).max()
    print("raw err", np.abs(z_raw - raw).max() / np.abs(raw).max(), "with priors err",
          np.abs(z_solve - (raw + add)).max() / scale)
    assert np.abs(z_raw - raw).max() <= 1e-12 * np.abs(raw).max()
    assert np.abs(z_solve - (raw + add)).max() <= 1e-12 * scale
    np.testing.assert_array_equal(z_again, z_raw)


# ---- 3. ignored priors: the empty effective set is the parent path --------------------------------
COV_KEYS = ("point_cov", "ext_cov", "intr_cov", "cam_full")


def _run(pkg, prob, setup, iters=6):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        setup(s)
        out = s.solve(_opts(pkg, iters))
        return out, s.covariance(full=True), s.covariance(full=True, intrinsics=True)
    finally:
        s.close()


def _same_run(name, a, pa, b, pb):
    assert costs(a[0]) == costs(b[0]) and records(a[0]) == records(b[0]), name
    for k in ("num_parameters", "num_residuals", "schur_assembly", "termination", "final_cost", "initial_cost"):
        assert a[0][k] == b[0][k], (name, k)
    assert [i["gradient_max_norm"] for i in a[0]["iterations"]] == [i["gradient_max_norm"] for i in b[0]["iterations"]]
    for k in ("points", "ext", "intr"):
        np.testing.assert_array_equal(getattr(pa, k), getattr(pb, k))
    for ca, cb in ((a[1], b[1]), (a[2], b[2])):
        assert ca["info"]["status"] == cb["info"]["status"], name
        for k in COV_KEYS:
            if k in ca and ca[k] is not None:
                np.testing.assert_array_equal(ca[k], cb[k])
        for k in ("num_parameters", "num_residuals", "cost"):
            assert ca["info"][k] == cb["info"][k], (name, k)


def test_ignored_priors_are_the_parent_path_bitwise(pkg, orc, gpu):
    base, groups = czr.CASES["rig6x20-mixed-masks"](pkg)   # groups [7, 0, 2, 5, 0, 4]: 1 and 4 stay constant, 5 has no distortion
    calib = zr.calib(base, groups)
    every = zr.calib(base, 7)
    masked_out = (np.array([4, 1], np.int32), base.intr[[4, 1]] + 0.5, np.repeat(np.eye(6)[None] * 40.0, 2, axis=0))
    frozen = base.copy()
    frozen.freeze_camera = True

    def set_then_clear(s):
        s.set_intrinsics_free(groups)
        s.set_intr_priors(*calib)
        assert s.get_intr_priors()[3] == len(calib[0]) == 3
        s.set_intr_priors(None)
        assert s.get_intr_priors()[0].size == 0

    def solve_then_clear(s):
        s.set_intrinsics_free(groups)
        s.set_intr_priors(*calib)
        first = s.solve(_opts(pkg, 3))
        assert first["num_residuals"] == 2 * base.num_obs + 18
        s.update_parameters(base.points, base.ext)
        s.update_intrinsics(base.intr)
        s.set_intr_priors(np.zeros(0, np.int32), np.zeros((0, 6)), np.zeros((0, 6, 6)))

    def free(s):
        s.set_intrinsics_free(groups)

    def with_priors(pri):
        def f(s):
            s.set_intrinsics_free(groups)
            s.set_intr_priors(*pri)
            assert s.get_intr_priors()[3] == 0
        return f

    def no_mask(s):  # an all-constant mask: the priors name constant intrinsics only
        s.set_intr_priors(*every)
        assert s.get_intr_priors()[3] == 0

    def zero_mask(s):
        s.set_intrinsics_free(np.zeros(base.intr.shape[0], np.uint8))
        s.set_intr_priors(*every)

    def frozen_set(s):
        s.set_intrinsics_free(7)
        s.set_intr_priors(*every)
        assert s.get_intr_priors()[3] == 0

    def _cov_free(prob, setup):
        # plain dab_covariance refuses a non-empty free set: run it before the mask is set
        s = pkg.Solver(0)
        try:
            s.set_problem(prob)
            setup(s)
            out = s.solve(_opts(pkg, 6))
            return out, s.covariance(full=True, intrinsics=True), s.covariance(full=True, intrinsics=True)
        finally:
            s.close()

    plain_p, free_p, frozen_p = base.copy(), base.copy(), frozen.copy()
    plain = _run(pkg, plain_p, lambda s: None)
    freed = _cov_free(free_p, free)
    froz = _run(pkg, frozen_p, lambda s: s.set_intrinsics_free(7))
    assert plain[1]["info"]["status"] == plain[2]["info"]["status"] == freed[1]["info"]["status"] == "OK"
    assert freed[0]["num_parameters"] == plain[0]["num_parameters"] + 10
    for name, start, setup, runner, want, want_p in (
            ("all-constant mask", base, no_mask, _run, plain, plain_p),
            ("zero mask", base, zero_mask, _run, plain, plain_p),
            ("freeze_camera", frozen, frozen_set, _run, froz, frozen_p),
            ("masked-out intrinsics named", base, with_priors(masked_out), _cov_free, freed, free_p),
            ("set, then cleared", base, set_then_clear, _cov_free, freed, free_p),
            ("solved, then cleared", base, solve_then_clear, _cov_free, freed, free_p)):
        p = start.copy()
        _same_run(name, runner(p, setup) if runner is _cov_free else runner(pkg, p, setup), p, want, want_p)


def test_prior_on_an_unreferenced_intrinsic_is_ignored(pkg, orc, gpu):
    prob, groups, ip, ignored = _eval_case(pkg, orc)
    keep = [j for j in range(len(ip[0])) if j not in ignored]
    only = tuple(x[keep] for x in ip)
    pa, pb = prob.copy(), prob.copy()
    a = gpu_solve(pkg, pa, ip, groups, 6)
    b = gpu_solve(pkg, pb, only, groups, 6)
    assert a["num_effective"] == b["num_effective"] == len(keep)
    assert costs(a) == costs(b) and records(a) == records(b) and a["num_residuals"] == b["num_residuals"]
    for k in ("points", "ext", "intr"):
        np.testing.assert_array_equal(getattr(pa, k), getattr(pb, k))
    np.testing.assert_array_equal(pa.intr[[2, 3, 7]], prob.intr[[2, 3, 7]])


def test_inactive_columns_and_entries_change_nothing_bitwise(pkg, orc, gpu):
    """shape_a, groups [5, 0, 2]: slots the model lacks and slots the mask leaves constant."""
    prob = ir.shape_a(pkg, orc)
    groups = np.array([5, 0, 2])
    idx, mu, A = zr.calib(prob, groups)
    act = lr.Layout(prob, None, groups).act[idx]
    rng = np.random.default_rng(5)
    mu2, A2 = mu.copy(), A.copy()
    mu2[~act] = 1e6 * rng.standard_normal((~act).sum())
    for j in range(len(idx)):
        A2[j][:, ~act[j]] = 1e3 * rng.standard_normal((6, (~act[j]).sum()))
    pa, pb = prob.copy(), prob.copy()
    a = gpu_solve(pkg, pa, (idx, mu, A), groups, 6)
    b = gpu_solve(pkg, pb, (idx, mu2, A2), groups, 6)
    assert costs(a) == costs(b) and records(a) == records(b) and a["initial_cost"] == b["initial_cost"]
    for k in ("points", "ext", "intr"):
        np.testing.assert_array_equal(getattr(pa, k), getattr(pb, k))


# ---- 4. state, errors, determinism ----------------------------------------------------------------
def test_prior_state_and_errors(pkg, orc, gpu):
    lib = pkg.load_library()
    start = ir.shape_b(pkg, orc)
    prob = start.copy()
    idx, mu, A = zr.calib(start, 7)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def raw(s, n, i, m, a):
        return lib.dab_set_intr_priors(s.h, n, None if i is None else i.ctypes.data_as(ip),
                                       None if m is None else m.ctypes.data_as(dp),
                                       None if a is None else a.ctypes.data_as(dp))

    def state(s):
        i, m, a, ne = s.get_intr_priors()
        return i.tobytes(), m.tobytes(), a.tobytes(), ne

    s = pkg.Solver(0)
    try:
        n = C.c_int32(-1)
        assert raw(s, 3, idx, mu, A) == -4  # DAB_E_STATE before dab_set_problem
        assert lib.dab_get_intr_priors(s.h, C.byref(n), None, None, None, None) == -4 and n.value == -1
        assert lib.dab_eval_intr_priors(s.h, None, None) == -4
        s.set_problem(prob)
        assert s.get_intr_priors()[0].size == 0 and s.get_intr_priors()[3] == 0
        s.set_intrinsics_free(7)
        s.set_intr_priors(idx, mu, A)
        want = state(s)
        assert want == (idx.tobytes(), mu.tobytes(), A.tobytes(), 12)
        cnt = len(idx)
        bad_idx, dup = idx.copy(), idx.copy()
        bad_idx[1] = start.intr.shape[0]
        dup[2] = dup[0]
        neg = idx.copy()
        neg[0] = -1
        nan_mu, inf_a = mu.copy(), A.copy()
        nan_mu[2, 4] = np.nan
        inf_a[1, 5, 5] = np.inf
        for name, args in (("count < 0", (-1, idx, mu, A)), ("null index", (cnt, None, mu, A)),
                           ("null mean", (cnt, idx, None, A)), ("null sqrt_info", (cnt, idx, mu, None)),
                           ("index out of range", (cnt, bad_idx, mu, A)), ("negative index", (cnt, neg, mu, A)),
                           ("duplicate", (cnt, dup, mu, A)), ("nan mean", (cnt, idx, nan_mu, A)),
                           ("inf sqrt_info", (cnt, idx, mu, inf_a))):
            assert raw(s, *args) == pkg.DAB_E_INVALID, name
            assert pkg.last_error() != ""
            assert state(s) == want, name
        assert lib.dab_set_intr_priors(None, cnt, idx.ctypes.data_as(ip), mu.ctypes.data_as(dp),
                                       A.ctypes.data_as(dp)) == pkg.DAB_E_INVALID
        first = s.solve(_opts(pkg, 6))
        assert first["num_residuals"] == 2 * start.num_obs + 72
        solved = (prob.points.copy(), prob.ext.copy(), prob.intr.copy())
        # kept by dab_update_parameters, dab_update_intrinsics, dab_set_loss, both masks and both other
        # prior calls: the same start walks the same path
        s.update_parameters(start.points, start.ext)
        s.update_intrinsics(start.intr)
        s.set_loss("trivial")
        s.set_intrinsics_free(0)
        assert s.get_intr_priors()[3] == 0           # the effective set follows the mask ...
        s.set_intrinsics_free(7)
        s.set_points_constant(None)
        s.set_ext_priors(None)
        s.set_point_priors(None)
        assert state(s) == want                       # ... and the priors stayed
        again = s.solve(_opts(pkg, 6))                # determinism: two solves are bitwise equal
        assert costs(again) == costs(first) and records(again) == records(first)
        assert [i["gradient_max_norm"] for i in again["iterations"]] == [i["gradient_max_norm"] for i in first["iterations"]]
        for got, w in zip((prob.points, prob.ext, prob.intr), solved):
            np.testing.assert_array_equal(got, w)
        # the order of setting changes nothing, bitwise
        perm = np.random.default_rng(2).permutation(cnt)
        s.update_parameters(start.points, start.ext)
        s.update_intrinsics(start.intr)
        s.set_intr_priors(idx[perm], mu[perm], A[perm])
        r_perm, c_perm = s.eval_intr_priors()
        permuted = s.solve(_opts(pkg, 6))
        assert costs(permuted) == costs(first) and records(permuted) == records(first)
        assert permuted["initial_cost"] == first["initial_cost"]
        for got, w in zip((prob.points, prob.ext, prob.intr), solved):
            np.testing.assert_array_equal(got, w)
        # a mask set after the priors changes the effective set at the next call
        s.update_parameters(start.points, start.ext)
        s.update_intrinsics(start.intr)
        s.set_intrinsics_free(czr.first(start, 5))
        assert s.get_intr_priors()[3] == 5
        five = s.solve(_opts(pkg, 2))
        assert five["num_residuals"] == 2 * start.num_obs + 30
        # reset by dab_set_problem
        p2 = start.copy()
        s.set_problem(p2)
        assert s.get_intr_priors()[0].size == 0 and s.get_intr_priors()[3] == 0
        s.set_intrinsics_free(7)
        free = s.solve(_opts(pkg, 6))
        assert free["num_residuals"] == 2 * start.num_obs and costs(free) != costs(first)
    finally:
        s.close()
    assert r_perm.shape == (cnt, 6) and c_perm > 0
    # core.solve's argument is the Solver's
    a = start.copy()
    ra = pkg.solve(a, max_iteration=6, free_intrinsics=7, intr_priors=(idx, mu, A), num_threads=4,
                   linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)
    assert costs(ra) == costs(first)
    np.testing.assert_array_equal(a.intr, solved[2])
    np.testing.assert_array_equal(a.ext, solved[1])


# ---- 5. dab_covariance_intrinsics ---------------------------------------------------------------
_cov_ref = {}


def cov_ref(pkg, orc, name):
    if name not in _cov_ref:
        prob, groups, ip = zr.thin_camera(pkg, 4) if name == "thin" else zr.cov_case(pkg, name)
        _cov_ref[name] = (prob, groups, ip, zr.covariance(pkg, orc, prob, groups=groups, intr_priors=ip))
    return _cov_ref[name]


def _cov(pkg, prob, groups, ip, solve_after=0):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        s.set_intrinsics_free(groups)
        if ip is not None:
            s.set_intr_priors(*ip)
        out = s.covariance(full=True, intrinsics=True)
        traj = s.solve(_opts(pkg, solve_after)) if solve_after else None
        return out, traj
    finally:
        s.close()


def _check_cov(tag, g, ref):
    assert g["info"]["status"] == "OK", g["info"]
    bound, m = czr.bound(ref)
    nan = np.isnan(ref["point_cov"])
    assert (np.isnan(g["point_cov"]) == nan).all()
    errs = {"point_cov": np.abs(np.where(nan, 0.0, g["point_cov"] - ref["point_cov"])).max()}
    for k in ("ext_cov", "intr_cov", "cam_full"):
        assert g[k].shape == ref[k].shape, k
        errs[k] = np.abs(g[k] - ref[k]).max()
    for k, e in errs.items():
        print(f"{tag}: {k} error {e:.3e} = {e / bound:.3g} of the bound {bound:.3e} (kappa {ref['kappa']:.3g}, "
              f"camera + z pivot ratio {g['info']['camera_pivot_ratio']:.3g})")
    for k, e in errs.items():
        assert e <= bound, (k, e, bound)
    assert g["info"]["num_parameters"] == ref["num_parameters"] and g["info"]["num_residuals"] == ref["num_residuals"]
    assert g["info"]["cost"] == pytest.approx(ref["cost"], rel=1e-12)
    full = g["cam_full"]
    assert (full == full.T).all()
    assert (g["intr_index"] == ref["intr_index"]).all()


@pytest.mark.parametrize("name", zr.COV_CASES)
def test_covariance_intrinsics_with_calibration_priors(pkg, orc, gpu, name):
    prob, groups, ip, ref = cov_ref(pkg, orc, name)
    assert not ref["rank"]["deficient"] and ref["num_effective"] == len(ip[0])
    assert ref["num_residuals"] == 2 * prob.num_obs + 6 * len(ip[0])
    g, traj = _cov(pkg, prob.copy(), groups, ip, solve_after=4)
    _check_cov(name + "/calib", g, ref)
    # the priors tighten it: against the covariance without them
    free, _ = _cov(pkg, prob.copy(), groups, None)
    vf = np.array([np.diag(x) for x in free["intr_cov"]])
    vg = np.array([np.diag(x) for x in g["intr_cov"]])
    assert (vg[vf > 0] / vf[vf > 0]).min() < 0.1 and free["info"]["num_residuals"] == 2 * prob.num_obs
    # a dab_solve after the covariance walks the trajectory it walks alone, bitwise
    alone = gpu_solve(pkg, prob.copy(), ip, groups, 4)
    assert costs(traj) == costs(alone) and records(traj) == records(alone)


def test_calibration_priors_cure_a_thin_camera(pkg, orc, gpu):
    """Camera 5 of bal40-first16 keeps 4 observations: 8 rows for 6 + 5 unknowns."""
    prob, groups, ip, ref = cov_ref(pkg, orc, "thin")
    assert not ref["rank"]["deficient"] and ref["rank"]["camera_ratio"] > 1e-6   # the reference passes its rank test
    s = pkg.Solver(0)
    try:
        s.set_problem(prob.copy())
        s.set_intrinsics_free(groups)
        nfe = int((prob.ext_const == 0).sum())
        n2 = 6 * nfe + 6 * 16
        arrs = [np.full((prob.points.shape[0], 6), SENTINEL), np.full((nfe, 21), SENTINEL), np.full((16, 21), SENTINEL),
                np.full((n2, n2), SENTINEL)]
        info, zinfo = pkg.DabCovarianceInfo(), pkg.DabCovarianceIntrInfo()
        ptr = [a.ctypes.data_as(C.POINTER(C.c_double)) for a in arrs]
        rc = s.lib.dab_covariance_intrinsics(s.h, None, *ptr, C.byref(info), C.byref(zinfo))
        print("thin camera without priors: status", info.status, "camera + z pivot ratio", info.camera_pivot_ratio)
        assert rc == 0 and info.status == 1 and info.num_free_ext == nfe and zinfo.num_free_intr == 16
        assert info.camera_pivot_ratio < 1e-10
        for a in arrs:
            assert (a == SENTINEL).all()         # no array written
        s.set_intr_priors(*ip)
        g = s.covariance(full=True, intrinsics=True)
    finally:
        s.close()
    _check_cov("thin camera/calib", g, ref)
    assert g["info"]["camera_pivot_ratio"] > 1e-6


# ---- 6. two ranks -------------------------------------------------------------------------------
def test_two_ranks_match_single_handle(gpu):
    """The test that catches a prior added once per rank: the priors' share of the initial cost is
    far above the script's tolerance (it checks that itself)."""
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
           "--free-intrinsics", "7", "--intr-priors", "calib", "--iters", "6", "--solvers", "explicit"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]
    assert '"rig_0"' in p.stdout and '"intr_prior_share"' in p.stdout


# ---- 7. the C++ host ----------------------------------------------------------------------------
def test_dam_set_intr_priors(pkg, orc, gpu):
    import importlib

    import deeparc_ref
    from golden_util import GOLDEN
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_rig.deeparc")
    prob = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    ip = zr.calib(prob, 7)
    nfree = len(ip[0])
    assert nfree == prob.intr.shape[0] > 0
    m = host.DeepArcManager()
    m.read(path)
    m.set_intrinsics_free(7)
    m.set_intr_priors(*ip)
    g = host.solve(m, max_iteration=10)
    p = pkg.solve(prob, max_iteration=10, free_intrinsics=7, intr_priors=ip)
    plain = pkg.solve(deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path)), max_iteration=10, free_intrinsics=7)
    assert g["num_residuals"] == p["num_residuals"] == 2 * prob.num_obs + 6 * nfree
    assert records(g) == records(p) and g["termination"] == p["termination"]
    np.testing.assert_allclose(costs(g), costs(p), rtol=1e-9, atol=0)
    assert abs(p["final_cost"] - plain["final_cost"]) > 1e-6 * plain["final_cost"]
    # a filter round changes the structure: the next solve re-sets the problem and applies the priors again
    r = orc.eval_residuals(pkg, prob)[0]
    m.filterPoint3d(float(np.median((r * r).sum(axis=1) / 2.0)), [0.0, 0.0, 0.0], 1e12)
    nblocks = len(m.blocks()[0])
    assert 0 < nblocks < prob.num_obs
    g2 = host.solve(m, max_iteration=3)
    extra = g2["num_residuals"] - 2 * nblocks
    assert extra % 6 == 0 and 0 < extra <= 6 * nfree   # (an intrinsic that lost every observation leaves the free set)
    # out of range: refused, the setting stays; then cleared
    with pytest.raises(RuntimeError):
        m.set_intr_priors(np.array([prob.intr.shape[0]], np.int32), np.zeros((1, 6)), np.eye(6)[None])
    assert host.solve(m, max_iteration=1)["num_residuals"] == 2 * nblocks + extra
    m.set_intr_priors(None)
    assert host.solve(m, max_iteration=1)["num_residuals"] == 2 * nblocks
