"""Gaussian priors on extrinsics on the GPU (dab_set_ext_priors) through dab_solve and the
covariances, against tests/prior_ref.py (pinned by tests/test_prior_ref.py, which also measures
the reference's own spread on every trajectory case: at most 6.1e-11 of the cost, 3e-12 of the
parameters, and that every case differs from its no-prior trajectory by at least 100 tolerances).

Tolerances are the project's: same iteration records, termination and num_residuals,
per-iteration cost 1e-9 relative, parameters 1e-7, intrinsics 1e-7 max(1, |v|); PCG run to
convergence against EXPLICIT 1e-6 (the rule of tests/test_gpu_robust.py and test_gpu_ptconst.py);
covariance blocks 64 kappa 2^-53 max|Sigma| (tests/test_gpu_covariance.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_ref as cr
import intr_ref as ir
import lm_ref as lr
import prior_ref as qr
import ptconst_ref as pr
import robust_ref as rr

pytestmark = pytest.mark.gpu

TRIVIAL = (rr.TRIVIAL, 1.0)
LOSS_NAME = {rr.TRIVIAL: None, rr.CAUCHY: "cauchy"}
TRAJ = {t[0]: t for t in qr.TRAJECTORIES}


def records(s):
    return [(i["success"], i["valid"]) for i in s["iterations"]]


def costs(s):
    return [i["cost"] for i in s["iterations"]]


def _opts(pkg, iters, lst=None, **kw):
    return pkg.options(max_num_iterations=iters, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR if lst is None else lst, **kw)


def gpu_solve(pkg, prob, priors, const=None, iters=25, loss=None, groups=0, lst=None, want_mf=None, **kw):
    s = pkg.Solver(0)
    try:
        if loss and loss[0] != rr.TRIVIAL:
            s.set_loss(LOSS_NAME[loss[0]], loss[1])
        s.set_problem(prob)
        if np.any(groups):
            s.set_intrinsics_free(groups)
        if const is not None:
            s.set_points_constant(const)
        if priors is not None:
            s.set_ext_priors(*priors)
        out = s.solve(_opts(pkg, iters, lst, **kw))
        out["num_effective"] = s.get_ext_priors()[3]
        if want_mf is not None:
            assert s.pcg_matrix_free() == want_mf
        return out
    finally:
        s.close()


_ref = {}


def reference(pkg, orc, key, make, iters, const=None, loss=None, groups=0):
    """(summary, solved problem, start, priors, mask) of lm_ref.lm, once per key, never modified.
    make() -> (problem, priors)."""
    if key not in _ref:
        start, priors = make()
        p = start.copy()
        m = pr.MASKS[const](p) if isinstance(const, str) else const
        _ref[key] = (lr.lm(pkg, orc, p, _opts(pkg, iters), priors=priors, const=m, groups=groups, loss=loss or TRIVIAL), p, start,
                     priors, m)
    return _ref[key]


def traj_ref(pkg, orc, name):
    t = TRAJ[name]

    def make():
        prob, priors, _, _, _, _ = qr.make_case(pkg, orc, t)
        return prob, priors
    return reference(pkg, orc, ("traj", name), make, t[6], t[3], t[4], t[5])


def check_against(tag, g, prob, ref, cost_tol=1e-9):
    o, pref, start, priors, m = ref
    err = max((abs(x - y) / abs(y) for x, y in zip(costs(g), costs(o))), default=0.0)
    print(tag, g["termination"], g["num_iterations"], "cost", g["initial_cost"], "->", g["final_cost"], "rejected",
          g["num_unsuccessful_steps"], "assembly", g["schur_assembly"], "max rel cost err", err, "points err",
          np.abs(prob.points - pref.points).max(), "ext err", np.abs(prob.ext - pref.ext).max(), "intr err",
          np.abs(prob.intr - pref.intr).max())
    assert g["termination"] == o["termination"], (g["message"], o["message"])
    assert g["num_iterations"] == o["num_iterations"]
    assert records(g) == records(o)
    assert g["num_residuals"] == o["num_residuals"]
    assert g["initial_cost"] == pytest.approx(o["initial_cost"], rel=1e-12)
    for x, y in zip(g["iterations"], o["iterations"]):
        assert abs(x["cost"] - y["cost"]) <= cost_tol * abs(y["cost"]), (x, y)
    assert np.abs(prob.points - pref.points).max() < 1e-7
    assert np.abs(prob.ext - pref.ext).max() < 1e-7
    assert (np.abs(prob.intr - pref.intr) <= 1e-7 * np.maximum(1.0, np.abs(pref.intr))).all()
    if m is not None:
        np.testing.assert_array_equal(prob.points[m], start.points[m])
    assert g["num_parameters"] == o["num_parameters"] and g["num_free_ext"] == o["num_free_ext"]


def run_traj(pkg, orc, name, **kw):
    t = TRAJ[name]
    ref = traj_ref(pkg, orc, name)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], ref[4], t[6], t[4], t[5], **kw)
    return g, prob, ref


# ---- 1. trajectories ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", [t[0] for t in qr.TRAJECTORIES[:9]])
def test_trajectory_matches_reference(pkg, orc, gpu, name):
    g, prob, ref = run_traj(pkg, orc, name)
    check_against(name, g, prob, ref)
    assert len(ref[0]["iterations"]) >= 6
    if name in qr.REJECTED:
        assert g["num_unsuccessful_steps"] > 0
    # "all": no free point, S = U + D^2 with the priors' A^T A inside U (block solves on B; the
    # rig's cross blocks take the dense branch of the same assembly)
    assert g["schur_assembly"] == (pkg.DAB_SCHUR_DIRECT if TRAJ[name][3] == "all" else pkg.DAB_SCHUR_TILES)
    assert g["num_effective"] == len(ref[3][0]) and g["num_residuals"] == 2 * prob.num_obs + 6 * g["num_effective"]


# ---- 2. both assemblies, the direct step, the pair tables at scale ------------------------------
@pytest.mark.parametrize("tiles", ["0", "1"])
@pytest.mark.parametrize("name", ["B-pose", "R-pos3"])
def test_trajectory_both_assemblies(pkg, orc, gpu, name, tiles, monkeypatch):
    monkeypatch.setenv("DAB_SCHUR_TILES", tiles)  # read when the handle is created
    g, prob, ref = run_traj(pkg, orc, name)
    check_against(f"{name}/tiles={tiles}", g, prob, ref)
    assert g["schur_assembly"] == int(tiles)


@pytest.mark.parametrize("name", ["B-pose-all", "R-pose-all"])
def test_direct_matches_general_masked_path(pkg, orc, gpu, name, monkeypatch):
    d, pd, ref = run_traj(pkg, orc, name)
    monkeypatch.setenv("DAB_POINTS_DIRECT", "0")
    g, pg, _ = run_traj(pkg, orc, name)
    print(name, "direct", d["schur_assembly"], d["final_cost"], "general", g["schur_assembly"], g["final_cost"],
          "max rel", max(abs(x - y) / abs(y) for x, y in zip(costs(d), costs(g))))
    assert d["schur_assembly"] == pkg.DAB_SCHUR_DIRECT
    assert g["schur_assembly"] in (pkg.DAB_SCHUR_PAIRS, pkg.DAB_SCHUR_TILES)
    assert records(d) == records(g) and d["termination"] == g["termination"]
    np.testing.assert_allclose(costs(d), costs(g), rtol=1e-9, atol=0)
    assert np.abs(pd.ext - pg.ext).max() < 1e-7
    check_against(name + "/general", g, pg, ref)


def _bal170(pkg):
    prob = cr.bal170(pkg)
    return prob, qr.pose(prob)


def test_bal170_pair_tables(pkg, orc, gpu):
    """168 free cameras (> 160: pair tables by selection); k_prior_blocks runs five rounds."""
    ref = reference(pkg, orc, ("bal170",), lambda: _bal170(pkg), 5)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], None, 5)
    check_against("bal170/pose", g, prob, ref)
    assert g["schur_assembly"] == pkg.DAB_SCHUR_PAIRS and g["num_free_ext"] == 168 == g["num_effective"]


# ---- 3. PCG -------------------------------------------------------------------------------------
def _low(pkg, case):
    prob = pr.case_b_low(pkg) if case == "B" else pr.case_r(pkg)
    return prob, qr.pose(prob)


PCG_FORMS = {  # case, environment, pcg_matrix_free()
    "R-matrix-free": ("R", {}, 1),
    "B-stored-y-fused": ("B", {"DAB_PCG_MF": "0", "DAB_PCG_FUSED": "1"}, 0),
    "B-stored-y-passes": ("B", {"DAB_PCG_MF": "0", "DAB_PCG_FUSED": "0"}, 0),
    "bal170-stored-y": ("bal170", {"DAB_PCG_MF": "0"}, 0),
}
_explicit = {}


def _explicit_run(pkg, case, iters):
    if case not in _explicit:
        start, priors = _bal170(pkg) if case == "bal170" else _low(pkg, case)
        p = start.copy()
        _explicit[case] = (gpu_solve(pkg, p, priors, None, iters), start, priors)
    return _explicit[case]


@pytest.mark.parametrize("form", list(PCG_FORMS))
def test_pcg_converged_matches_explicit(pkg, gpu, form, monkeypatch):
    case, env, mf = PCG_FORMS[form]
    e, start, priors = _explicit_run(pkg, case, 5)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pp = start.copy()
    p = gpu_solve(pkg, pp, priors, None, 5, lst=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG, eta=1e-14,
                  max_linear_solver_iterations=1000, want_mf=mf)
    print(form, "explicit", repr(e["final_cost"]), "pcg", repr(p["final_cost"]), "assembly", p["schur_assembly"],
          "max rel", max(abs(x - y) / abs(y) for x, y in zip(costs(p), costs(e))))
    assert records(e) == records(p) and p["num_residuals"] == e["num_residuals"]
    np.testing.assert_allclose(costs(p), costs(e), rtol=1e-6, atol=0)
    # and the priors are in both: without them the explicit solve ends far more than 1e-6 away
    plain = gpu_solve(pkg, start.copy(), None, None, 5)
    print(form, "final cost without priors", repr(plain["final_cost"]))
    assert abs(plain["final_cost"] - e["final_cost"]) > 1e-4 * e["final_cost"]


def _parity_shape(pkg, kind):
    """The shapes of test_gpu_parity.py::test_matrix_free_mixed_precision_pcg_matches_oracle."""
    if kind == "bal":
        return pkg.synth(kind=0, num_cameras=60, num_points=4000, obs_per_point=7, seed=61)
    return pkg.synth(kind=1, num_arcs=6, num_rings=16, num_points=3000, obs_per_point=8, seed=62)


@pytest.mark.parametrize("kind,env,mf", [("rig", {}, 2), ("bal", {}, 2), ("bal", {"DAB_PCG_MF": "0"}, 0)])
def test_pcg_fp32_matches_fp64_pcg(pkg, gpu, kind, env, mf, monkeypatch):
    """pcg_fp32 with pose priors against the fp64 PCG at the same (default) settings: equal CG counts,
    per-iteration cost 1e-6, the mixed-precision rule of tests/test_gpu_parity.py on that rule's own
    shapes, 12 iterations: matrix-free fp32 products on both, fp32 Y records on the BAL one. (U, g_c
    and the costs, where the priors enter, are fp64 on these paths.) Measured: 1.4e-7, 1.2e-10 and
    2.3e-11, as without priors (1.6e-7, 1.3e-10, 3.3e-11). The 4 x 6 rig R of the other tests cannot
    carry this rule: from its initial cost of 7.7e9 the fp32 products alone, without any prior, move
    the fifth cost by 1.2e-4 (7.1e-5 with priors)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    start = _parity_shape(pkg, kind)
    priors = qr.pose(start)
    kw = dict(lst=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG)
    a = gpu_solve(pkg, start.copy(), priors, None, 12, pcg_fp32=0, want_mf=min(mf, 1), **kw)
    b = gpu_solve(pkg, start.copy(), priors, None, 12, pcg_fp32=1, want_mf=mf, **kw)
    cg = [[i["linear_solver_iterations"] for i in s["iterations"]] for s in (a, b)]
    print(kind, env, "fp64", repr(a["final_cost"]), "fp32", repr(b["final_cost"]), "cg", cg, "max rel",
          max(abs(x - y) / abs(y) for x, y in zip(costs(b), costs(a))))
    assert cg[0] == cg[1] and records(a) == records(b) and max(cg[0]) > 1
    assert a["num_residuals"] == b["num_residuals"] == 2 * start.num_obs + 6 * len(priors[0])
    np.testing.assert_allclose(costs(b), costs(a), rtol=1e-6, atol=0)


# ---- 4. combinations ----------------------------------------------------------------------------
@pytest.mark.parametrize("lds", ["1", "0"])
def test_free_intrinsics_with_priors(pkg, orc, gpu, lds, monkeypatch):
    monkeypatch.setenv("DAB_INTR_BORDER_LDS", lds)
    g, prob, ref = run_traj(pkg, orc, "A-pose-groups7")
    check_against(f"shape_a/groups 7/pose/lds={lds}", g, prob, ref)
    assert np.abs(prob.intr - ref[2].intr).max() > 1e-3
    assert g["num_parameters"] == 3 * g["num_free_points"] + 6 * g["num_free_ext"] + 13


def test_constant_points_and_loss(pkg, orc, gpu):
    g, prob, ref = run_traj(pkg, orc, "B-pose-third-cauchy")
    check_against("B/pose/third/cauchy", g, prob, ref)
    assert g["num_free_points"] == int((~ref[4]).sum())


def _same(a, b, pa, pb):
    assert costs(a) == costs(b) and records(a) == records(b)
    for k in ("num_parameters", "num_residuals", "num_free_ext", "schur_assembly", "termination", "final_cost",
              "initial_cost"):
        assert a[k] == b[k], k
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)


def test_freeze_camera_ignores_priors(pkg, gpu):
    start = pr.case_b(pkg)
    priors = qr.pose(start)
    start.freeze_camera = True
    pa, pb = start.copy(), start.copy()
    a = gpu_solve(pkg, pa, priors, None, 8)
    b = gpu_solve(pkg, pb, None, None, 8)
    assert a["num_effective"] == 0 and a["num_residuals"] == 2 * start.num_obs
    _same(a, b, pa, pb)
    np.testing.assert_array_equal(pa.ext, start.ext)


def test_priors_on_constant_and_unreferenced_extrinsics_are_ignored(pkg, gpu):
    base = pr.case_b(pkg)
    unref = 5
    start = base.subset(base.obs_ext0 != unref).copy()   # camera 5 is referenced by no observation
    assert start.ext_const[0] and not (start.obs_ext0 == unref).any()
    idx, mu, A = qr.pose(start)
    assert 0 not in idx and unref not in idx
    rng = np.random.default_rng(4)
    extra = (np.concatenate([idx, [0, unref]]).astype(np.int32),
             np.concatenate([mu, start.ext[[0, unref]] + 0.1]), np.concatenate([A, 30.0 * rng.standard_normal((2, 6, 6))]))
    pa, pb = start.copy(), start.copy()
    a = gpu_solve(pkg, pa, extra, None, 8)
    b = gpu_solve(pkg, pb, (idx, mu, A), None, 8)
    assert a["num_effective"] == b["num_effective"] == len(idx)
    _same(a, b, pa, pb)
    np.testing.assert_array_equal(pa.ext[[0, unref]], start.ext[[0, unref]])


# ---- 5. the empty effective set is the parent path ----------------------------------------------
COV_KEYS = ("point_cov", "ext_cov", "ext_full")


def _run(pkg, prob, setup, iters=8):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        setup(s)
        out = s.solve(_opts(pkg, iters))
        return out, s.covariance(full=True)
    finally:
        s.close()


def test_empty_effective_set_is_the_parent_path_bitwise(pkg, gpu):
    base = cr.bal40(pkg)  # cameras 0 and 1 constant
    pose = qr.pose(base)
    plain_p = base.copy()
    plain, plain_cov = _run(pkg, plain_p, lambda s: None)
    assert plain_cov["info"]["status"] == "OK"
    const_only = (np.array([1, 0], np.int32), base.ext[[1, 0]] + 0.5, np.repeat(np.eye(6)[None] * 40.0, 2, axis=0))

    def set_then_clear(s):
        s.set_ext_priors(*pose)
        assert s.get_ext_priors()[3] == len(pose[0]) == 38
        s.set_ext_priors(None)
        assert s.get_ext_priors()[0].size == 0

    def solve_then_clear(s):
        s.set_ext_priors(*pose)
        first = s.solve(_opts(pkg, 3))
        assert first["num_residuals"] == 2 * base.num_obs + 6 * 38
        s.update_parameters(base.points, base.ext)
        s.set_ext_priors(np.zeros(0, np.int32), np.zeros((0, 6)), np.zeros((0, 6, 6)))

    for name, setup in (("count 0", lambda s: s.set_ext_priors(None)), ("constant only", lambda s: s.set_ext_priors(*const_only)),
                        ("cleared", set_then_clear), ("solved, then cleared", solve_then_clear)):
        p = base.copy()
        out, cov = _run(pkg, p, setup)
        assert costs(out) == costs(plain) and records(out) == records(plain), name
        for k in ("num_parameters", "num_residuals", "schur_assembly", "termination", "final_cost", "initial_cost"):
            assert out[k] == plain[k], (name, k)
        np.testing.assert_array_equal(p.points, plain_p.points)
        np.testing.assert_array_equal(p.ext, plain_p.ext)
        for k in COV_KEYS:
            np.testing.assert_array_equal(cov[k], plain_cov[k])
        for k in ("num_parameters", "num_residuals", "cost"):
            assert cov["info"][k] == plain_cov["info"][k], (name, k)


# ---- 6. dab_eval_ext_priors ---------------------------------------------------------------------
@pytest.mark.parametrize("case,loss", [("B", None), ("R", pr.CAUCHY2)])
def test_eval_ext_priors_against_numpy(pkg, orc, gpu, case, loss):
    prob = pr.CASES[case](pkg)
    idx, mu, A = qr.pose(prob)
    # camera 0 / arc 0 is constant: its prior is ignored, its row is zero
    idx = np.concatenate([[0], idx]).astype(np.int32)
    mu = np.concatenate([prob.ext[[0]] + 1.0, mu])
    A = np.concatenate([np.eye(6)[None], A])
    s = pkg.Solver(0)
    try:
        if loss:
            s.set_loss(LOSS_NAME[loss[0]], loss[1])
        s.set_problem(prob)
        s.set_ext_priors(idx, mu, A)
        r, cost = s.eval_ext_priors()
        want = np.einsum("nij,nj->ni", A, prob.ext[idx] - mu)
        want[0] = 0.0
        want_cost = 0.5 * (want * want).sum()
        print(case, "residual err", np.abs(r - want).max(), "of", np.abs(want).max(), "cost", cost, want_cost)
        assert np.abs(r - want).max() <= 1e-12 * np.abs(want).max()
        assert cost == pytest.approx(want_cost, rel=1e-12)
        raw_r, raw_cost = s.residuals()          # raw observation quantities: no prior in them
        assert raw_cost == pytest.approx(0.5 * (raw_r * raw_r).sum(), rel=1e-12)
        out = s.solve(_opts(pkg, 2))
        # 0.5 sum rho of the observations (never the prior under the loss) + the prior cost
        rho_cost = rr.cost(*(loss or TRIVIAL), orc.eval_residuals(pkg, pr.CASES[case](pkg))[0])
        assert out["initial_cost"] == pytest.approx(rho_cost + want_cost, rel=1e-12)
        assert out["num_residuals"] == 2 * prob.num_obs + 6 * (len(idx) - 1)
        assert s.get_ext_priors()[3] == len(idx) - 1
    finally:
        s.close()


# ---- 7. state, errors, determinism --------------------------------------------------------------
def test_prior_state_and_errors(pkg, gpu):
    lib = pkg.load_library()
    start = pr.case_b(pkg)
    prob = start.copy()
    idx, mu, A = qr.pos3(start)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def raw(s, n, i, m, a):
        return lib.dab_set_ext_priors(s.h, n, None if i is None else i.ctypes.data_as(ip),
                                      None if m is None else m.ctypes.data_as(dp),
                                      None if a is None else a.ctypes.data_as(dp))

    def state(s):
        i, m, a, ne = s.get_ext_priors()
        return i.tobytes(), m.tobytes(), a.tobytes(), ne

    s = pkg.Solver(0)
    try:
        n = C.c_int32(-1)
        assert raw(s, 3, idx, mu, A) == -4  # DAB_E_STATE before dab_set_problem
        assert lib.dab_get_ext_priors(s.h, C.byref(n), None, None, None, None) == -4 and n.value == -1
        assert lib.dab_eval_ext_priors(s.h, None, None) == -4
        s.set_problem(prob)
        assert s.get_ext_priors()[0].size == 0 and s.get_ext_priors()[3] == 0
        s.set_ext_priors(idx, mu, A)
        want = state(s)
        assert want == (idx.tobytes(), mu.tobytes(), A.tobytes(), 3)
        bad_idx, dup = idx.copy(), idx.copy()
        bad_idx[1] = start.ext.shape[0]
        dup[2] = dup[0]
        neg = idx.copy()
        neg[0] = -1
        nan_mu, inf_a = mu.copy(), A.copy()
        nan_mu[2, 4] = np.nan
        inf_a[1, 5, 5] = np.inf
        for name, args in (("count < 0", (-1, idx, mu, A)), ("null index", (3, None, mu, A)),
                           ("null mean", (3, idx, None, A)), ("null sqrt_info", (3, idx, mu, None)),
                           ("index out of range", (3, bad_idx, mu, A)), ("negative index", (3, neg, mu, A)),
                           ("duplicate", (3, dup, mu, A)), ("nan mean", (3, idx, nan_mu, A)),
                           ("inf sqrt_info", (3, idx, mu, inf_a))):
            assert raw(s, *args) == pkg.DAB_E_INVALID, name
            assert pkg.last_error() != ""
            assert state(s) == want, name
        assert lib.dab_set_ext_priors(None, 3, idx.ctypes.data_as(ip), mu.ctypes.data_as(dp),
                                      A.ctypes.data_as(dp)) == pkg.DAB_E_INVALID
        first = s.solve(_opts(pkg, 6))
        assert first["num_residuals"] == 2 * start.num_obs + 18
        solved = (prob.points.copy(), prob.ext.copy())
        # kept by dab_update_parameters, dab_set_loss and both masks: the same start walks the same path
        s.update_parameters(start.points, start.ext)
        s.set_loss("trivial")
        s.set_intrinsics_free(0)
        s.set_points_constant(None)
        assert state(s) == want
        again = s.solve(_opts(pkg, 6))            # determinism: two solves are bitwise equal
        assert costs(again) == costs(first) and records(again) == records(first)
        assert [i["gradient_max_norm"] for i in again["iterations"]] == [i["gradient_max_norm"] for i in first["iterations"]]
        np.testing.assert_array_equal(prob.points, solved[0])
        np.testing.assert_array_equal(prob.ext, solved[1])
        # reset by dab_set_problem
        p2 = start.copy()
        s.set_problem(p2)
        assert s.get_ext_priors()[0].size == 0 and s.get_ext_priors()[3] == 0
        free = s.solve(_opts(pkg, 6))
        assert free["num_residuals"] == 2 * start.num_obs and costs(free) != costs(first)
    finally:
        s.close()
    # core.solve's argument is the Solver's
    a = start.copy()
    ra = pkg.solve(a, max_iteration=6, ext_priors=(idx, mu, A), num_threads=4)
    assert costs(ra) == costs(first)
    np.testing.assert_array_equal(a.ext, solved[1])


# ---- 8. covariance ------------------------------------------------------------------------------
def _cov(pkg, prob, priors, groups=None, solve_after=0):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        if groups is not None:
            s.set_intrinsics_free(groups)
        if priors is not None:
            s.set_ext_priors(*priors)
        out = s.covariance(full=True, intrinsics=groups is not None)
        traj = s.solve(_opts(pkg, solve_after)) if solve_after else None
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
    assert g["info"]["num_parameters"] == ref["num_parameters"] and g["info"]["num_residuals"] == ref["num_residuals"]
    assert g["info"]["cost"] == pytest.approx(ref["cost"], rel=1e-12)
    full = g[full_key]
    assert (full == full.T).all()


@pytest.mark.parametrize("name", ["bal40", "rig3x5"])
def test_position_priors_fix_the_gauge(pkg, orc, gpu, name):
    prob = (cr.bal40 if name == "bal40" else cr.rig3x5)(pkg, ())
    priors = qr.pos3(prob, seed=3)
    free, _ = _cov(pkg, prob.copy(), None)
    assert free["info"]["status"] == "RANK_DEFICIENT" and free["point_cov"] is None
    ref = lr.covariance(pkg, orc, prob, priors=priors)
    assert not ref["rank"]["deficient"] and ref["num_effective"] == 3
    g, traj = _cov(pkg, prob.copy(), priors, solve_after=5)
    _check_cov(name + "/pos3", g, ref, "ext_full")
    assert g["info"]["camera_pivot_ratio"] > cr.MIN_PIVOT_RATIO
    # a dab_solve after the covariance walks the trajectory it walks without it, bitwise
    alone = gpu_solve(pkg, prob.copy(), priors, None, 5)
    assert costs(traj) == costs(alone) and records(traj) == records(alone)


def test_covariance_intrinsics_with_pose_priors(pkg, orc, gpu):
    prob = ir.shape_a(pkg, orc)
    priors = qr.pose(prob, seed=3)
    ref = lr.covariance(pkg, orc, prob, priors=priors, groups=7)
    assert not ref["rank"]["deficient"]
    g, traj = _cov(pkg, prob.copy(), priors, 7, solve_after=5)
    _check_cov("shape_a/groups 7/pose", g, ref, "cam_full")
    assert g["info"]["num_free_scalars"] == ref["num_free_scalars"] == 13
    alone = gpu_solve(pkg, prob.copy(), priors, None, 5, groups=7)
    assert costs(traj) == costs(alone) and records(traj) == records(alone)


# ---- 9. two ranks -------------------------------------------------------------------------------
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
           "--ext-priors", "pose", "--iters", "6", "--solvers", "explicit,pcg"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]
    assert '"bal_0"' in p.stdout and '"rig_0"' in p.stdout and '"prior_share"' in p.stdout


# ---- 10. the C++ host ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rig", "bal"])
def test_dam_set_ext_priors(pkg, orc, gpu, kind):
    import importlib

    import deeparc_ref
    from golden_util import GOLDEN
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_%s.deeparc" % kind)
    prob = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    priors = qr.pose(prob)
    nfree = len(priors[0])
    # with the constant extrinsic named too: ignored
    gauge = int(np.flatnonzero(prob.ext_const)[0])
    named = (np.concatenate([priors[0], [gauge]]).astype(np.int32), np.concatenate([priors[1], prob.ext[[gauge]] + 1.0]),
             np.concatenate([priors[2], np.eye(6)[None]]))
    m = host.DeepArcManager()
    m.read(path)
    m.set_ext_priors(*named)
    g = host.solve(m, max_iteration=10)
    p = pkg.solve(prob, max_iteration=10, ext_priors=priors)
    plain = pkg.solve(deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path)), max_iteration=10)
    assert g["num_residuals"] == p["num_residuals"] == 2 * prob.num_obs + 6 * nfree
    assert records(g) == records(p) and g["termination"] == p["termination"]
    np.testing.assert_allclose(costs(g), costs(p), rtol=1e-9, atol=0)
    assert abs(p["final_cost"] - plain["final_cost"]) > 1e-6 * plain["final_cost"]
    xyz, _ = m.points()
    cams, _ = m.cameras()
    np.testing.assert_allclose(xyz, prob.points, rtol=0, atol=1e-7)
    np.testing.assert_allclose(cams, prob.ext, rtol=0, atol=1e-7)
    # a filter round changes the structure: the next solve re-sets the problem and applies the priors again
    # (filterPoint3d drops the observations below the bound: the median keeps about half)
    r = orc.eval_residuals(pkg, prob)[0]
    m.filterPoint3d(float(np.median((r * r).sum(axis=1) / 2.0)), [0.0, 0.0, 0.0], 1e12)
    nblocks = len(m.blocks()[0])
    assert 0 < nblocks < prob.num_obs
    g2 = host.solve(m, max_iteration=3)
    # (an extrinsic that lost every observation leaves the free set, and its prior with it)
    assert g2["num_residuals"] == 2 * nblocks + 6 * g2["num_free_ext"] and 0 < g2["num_free_ext"] <= nfree
    nfree = g2["num_free_ext"]
    # out of range: refused, the setting stays; then cleared
    with pytest.raises(RuntimeError):
        m.set_ext_priors(np.array([prob.ext.shape[0]], np.int32), np.zeros((1, 6)), np.eye(6)[None])
    assert host.solve(m, max_iteration=1)["num_residuals"] == 2 * nblocks + 6 * nfree
    m.set_ext_priors(None)
    assert host.solve(m, max_iteration=1)["num_residuals"] == 2 * nblocks
