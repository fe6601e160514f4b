"""Gaussian priors on points on the GPU (dab_set_point_priors) through dab_solve and the covariances,
against tests/ptprior_ref.py (pinned by tests/test_ptprior_ref.py, which also asserts the reference's
own spread on every trajectory case, at most 1e-10 of the cost and 1e-8 of the parameters, and that
every case differs from its no-prior trajectory by at least 100 tolerances).

Tolerances are the project's: same iteration records, termination and num_residuals,
per-iteration cost 1e-9 relative, parameters 1e-7, intrinsics 1e-7 max(1, |v|); PCG run to
convergence against EXPLICIT 1e-6; pcg_fp32 against fp64 PCG: equal CG counts, cost 1e-6;
covariance blocks 64 kappa 2^-53 max|Sigma| (tests/test_gpu_covariance.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_ref as cr
import lm_ref as lr
import prior_ref as qr
import ptconst_ref as pr
import ptprior_ref as ppr
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


def gpu_solve(pkg, prob, point_priors, ext_priors=None, const=None, iters=25, loss=None, groups=0, lst=None,
              want_mf=None, **kw):
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
        out = s.solve(_opts(pkg, iters, lst, **kw))
        out["num_effective"] = s.get_point_priors()[3]
        if want_mf is not None:
            assert s.pcg_matrix_free() == want_mf
        return out
    finally:
        s.close()


_ref = {}


def reference(pkg, orc, key, make, iters, loss=None, groups=0):
    """(summary, solved problem, start, point priors, extrinsic priors, mask) of ptprior_ref.lm, once
    per key, never modified. make() -> (problem, point priors, extrinsic priors, mask)."""
    if key not in _ref:
        start, pp, ep, m = make()
        p = start.copy()
        out = ppr.lm(pkg, orc, p, _opts(pkg, iters), priors=ep, point_priors=pp, const=m, groups=groups,
                     loss=loss or TRIVIAL)
        _ref[key] = (out, p, start, pp, ep, m)
    return _ref[key]


def traj_ref(pkg, orc, name):
    t = ppr.TRAJ[name]
    prob, pp, ep, m, loss, groups, iters = ppr.make_case(pkg, orc, t)
    return reference(pkg, orc, ("traj", name), lambda: (prob, pp, ep, m), iters, loss, groups)


def check_against(tag, g, prob, ref, cost_tol=1e-9):
    o, pref, start, pp, ep, m = ref
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
    assert g["num_free_points"] == o["num_free_points"]


def run_traj(pkg, orc, name, **kw):
    t = ppr.TRAJ[name]
    ref = traj_ref(pkg, orc, name)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], ref[4], ref[5], t[7], t[5], t[6], **kw)
    return g, prob, ref


# ---- 1. trajectories ----------------------------------------------------------------------------
# the route every case takes by default: 168 free cameras take the pair tables by selection, the
# others the tiles; freeze_camera has no camera system at all (the per-point 3x3 step)
PAIRS_BY_DEFAULT = ("bal170-all",)


@pytest.mark.parametrize("name", [t[0] for t in ppr.TRAJECTORIES])
def test_trajectory_matches_reference(pkg, orc, gpu, name):
    g, prob, ref = run_traj(pkg, orc, name)
    check_against(name, g, prob, ref)
    t = ppr.TRAJ[name]
    if name in ppr.REJECTED:
        assert g["num_unsuccessful_steps"] > 0
    assert g["linear_solver_type_used"] == pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR
    if t[8]:
        assert g["num_free_ext"] == 0 and g["num_parameters"] == 3 * g["num_free_points"]
        np.testing.assert_array_equal(prob.ext, ref[2].ext)
    else:
        assert g["schur_assembly"] == (pkg.DAB_SCHUR_PAIRS if name in PAIRS_BY_DEFAULT else pkg.DAB_SCHUR_TILES)
    neff = len(ppr.pt_effective(lr.Layout(ref[2], ref[5], t[6]), ref[3]))
    assert g["num_effective"] == neff > 0
    assert g["num_residuals"] == 2 * prob.num_obs + 3 * neff + 6 * (len(ref[4][0]) if ref[4] else 0)
    if t[4]:  # the mask: some priors sit on constant points and are ignored
        assert neff < len(ref[3][0])


@pytest.mark.parametrize("tiles", ["0", "1"])
@pytest.mark.parametrize("name", ["B-all", "rig3x5-gcp3", "noise0"])
def test_trajectory_both_assemblies(pkg, orc, gpu, name, tiles, monkeypatch):
    """EXPLICIT with pair tables and with tiles. noise0 on the tiles is the case whose fixed-point
    rhs exponent overflows when it is taken from the observations' cost alone."""
    monkeypatch.setenv("DAB_SCHUR_TILES", tiles)  # read when the handle is created
    g, prob, ref = run_traj(pkg, orc, name)
    check_against(f"{name}/tiles={tiles}", g, prob, ref)
    assert g["schur_assembly"] == int(tiles)


# ---- 2. PCG -------------------------------------------------------------------------------------
def _low(pkg, case):
    prob = pr.case_b_low(pkg) if case == "B" else pr.case_r(pkg)
    return prob, ppr.all_points(prob)


PCG_FORMS = {  # case, environment, pcg_matrix_free()
    "R-matrix-free": ("R", {}, 1),
    "B-stored-y": ("B", {"DAB_PCG_MF": "0"}, 0),
}
_explicit = {}


def _explicit_run(pkg, case, iters):
    if case not in _explicit:
        start, pp = _low(pkg, case)
        _explicit[case] = (gpu_solve(pkg, start.copy(), pp, iters=iters), start, pp)
    return _explicit[case]


@pytest.mark.parametrize("form", list(PCG_FORMS))
def test_pcg_converged_matches_explicit(pkg, gpu, form, monkeypatch):
    case, env, mf = PCG_FORMS[form]
    e, start, pp = _explicit_run(pkg, case, 5)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = gpu_solve(pkg, start.copy(), pp, iters=5, lst=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG, eta=1e-14,
                  max_linear_solver_iterations=1000, want_mf=mf)
    print(form, "explicit", repr(e["final_cost"]), "pcg", repr(p["final_cost"]), "assembly", p["schur_assembly"],
          "max rel", max(abs(x - y) / abs(y) for x, y in zip(costs(p), costs(e))))
    assert records(e) == records(p) and p["num_residuals"] == e["num_residuals"]
    assert p["linear_solver_type_used"] == pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG
    np.testing.assert_allclose(costs(p), costs(e), rtol=1e-6, atol=0)
    # and the priors are in both: without them the explicit solve ends far more than 1e-6 away
    plain = gpu_solve(pkg, start.copy(), None, iters=5)
    assert abs(plain["final_cost"] - e["final_cost"]) > 1e-4 * e["final_cost"]


def _parity_shape(pkg, kind):
    """The shapes of test_gpu_parity.py::test_matrix_free_mixed_precision_pcg_matches_oracle."""
    if kind == "bal":
        return pkg.synth(kind=0, num_cameras=60, num_points=4000, obs_per_point=7, seed=61)
    return pkg.synth(kind=1, num_arcs=6, num_rings=16, num_points=3000, obs_per_point=8, seed=62)


@pytest.mark.parametrize("kind,env,mf", [("rig", {}, 2), ("bal", {}, 2), ("bal", {"DAB_PCG_MF": "0"}, 0)])
def test_pcg_fp32_matches_fp64_pcg(pkg, gpu, kind, env, mf, monkeypatch):
    """pcg_fp32 with a prior on every point against the fp64 PCG at the same (default) settings: equal
    CG counts, per-iteration cost 1e-6 (V, g and the costs, where the priors enter, are fp64)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    start = _parity_shape(pkg, kind)
    pp = ppr.all_points(start)
    kw = dict(lst=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG)
    a = gpu_solve(pkg, start.copy(), pp, iters=12, pcg_fp32=0, want_mf=min(mf, 1), **kw)
    b = gpu_solve(pkg, start.copy(), pp, iters=12, pcg_fp32=1, want_mf=mf, **kw)
    cg = [[i["linear_solver_iterations"] for i in s["iterations"]] for s in (a, b)]
    print(kind, env, "fp64", repr(a["final_cost"]), "fp32", repr(b["final_cost"]), "cg", cg, "max rel",
          max(abs(x - y) / abs(y) for x, y in zip(costs(b), costs(a))))
    assert cg[0] == cg[1] and records(a) == records(b) and max(cg[0]) > 1
    assert a["num_residuals"] == b["num_residuals"] == 2 * start.num_obs + 3 * len(pp[0])
    np.testing.assert_allclose(costs(b), costs(a), rtol=1e-6, atol=0)


# ---- 3. launch geometry of the new kernels ------------------------------------------------------
def _edge_shape(pkg):
    """600 points (more than two work-groups of 256 priors, no multiple of 64) x 4, 12 cameras."""
    return pkg.synth(kind=0, num_cameras=12, num_points=600, obs_per_point=4, seed=9, rot_noise=0.05,
                     trans_noise=0.1, point_noise=0.01)


def _first(pp, idx):
    return pp[0][idx], pp[1][idx], pp[2][idx]


EDGES = {  # which of the 600 priors: one; one below, at and one above a work-group; both ends; all
    "one": [300], "255": range(255), "256": range(256), "257": range(257), "ends": [0, 599], "every": range(600),
}


@pytest.mark.parametrize("edge", list(EDGES))
def test_launch_geometry_edges(pkg, orc, gpu, edge):
    """One prior, one arriving work-group and several, the first and the last point (whatever the
    device order of the points is, `every` covers device point 0 and the last of NP = 600), each
    against the reference; and the same set in another caller order solves bitwise the same."""
    start = _edge_shape(pkg)
    assert start.points.shape[0] == 600 and len(ppr.referenced(start)) == 600
    pp = _first(ppr.all_points(start), np.array(list(EDGES[edge])))
    ref = reference(pkg, orc, ("edge", edge), lambda: (start, pp, None, None), 4)
    prob = start.copy()
    g = gpu_solve(pkg, prob, pp, iters=4)
    check_against("edge/" + edge, g, prob, ref)
    assert g["num_effective"] == len(pp[0]) and g["num_residuals"] == 2 * start.num_obs + 3 * len(pp[0])
    perm = np.random.default_rng(3).permutation(len(pp[0]))
    p2 = start.copy()
    g2 = gpu_solve(pkg, p2, _first(pp, perm), iters=4)
    assert costs(g2) == costs(g) and records(g2) == records(g)
    np.testing.assert_array_equal(p2.points, prob.points)
    np.testing.assert_array_equal(p2.ext, prob.ext)


# ---- 4. covariance ------------------------------------------------------------------------------
def _cov(pkg, prob, pp, groups=None, solve_after=0):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        if groups is not None:
            s.set_intrinsics_free(groups)
        if pp is not None:
            s.set_point_priors(*pp)
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
def test_ground_control_fixes_the_gauge(pkg, orc, gpu, name):
    prob = ppr.shape(pkg, orc, name)
    pp = ppr.gcp3(prob, ppr.truth(pkg, name))
    free, _ = _cov(pkg, prob.copy(), None)
    assert free["info"]["status"] == "RANK_DEFICIENT" and free["point_cov"] is None
    ref = ppr.covariance(pkg, orc, prob, point_priors=pp)
    assert not ref["rank"]["deficient"] and ref["num_effective"] == 3
    g, traj = _cov(pkg, prob.copy(), pp, solve_after=5)
    _check_cov(name + "/gcp3", g, ref, "ext_full")
    assert g["info"]["camera_pivot_ratio"] > cr.MIN_PIVOT_RATIO
    # the control points' own covariance is about the prior's: they are known to sigma, not exactly
    sd = np.sqrt(np.diagonal(g["point_cov"][pp[0]], axis1=1, axis2=2))
    assert (sd > 0.1 * ppr.SIG_GCP).all() and (sd <= ppr.SIG_GCP).all()
    # a dab_solve after the covariance walks the trajectory it walks without it, bitwise
    alone = gpu_solve(pkg, prob.copy(), pp, iters=5)
    assert costs(traj) == costs(alone) and records(traj) == records(alone)


def test_covariance_intrinsics_with_point_priors(pkg, orc, gpu):
    prob = ppr.shape(pkg, orc, "A")
    pp = ppr.all_points(prob, seed=3)
    ref = ppr.covariance(pkg, orc, prob, point_priors=pp, groups=7)
    assert not ref["rank"]["deficient"]
    g, _ = _cov(pkg, prob.copy(), pp, 7)
    _check_cov("shape_a/groups 7/all", g, ref, "cam_full")
    assert g["info"]["num_free_scalars"] == ref["num_free_scalars"] == 13


def test_point_rank_test_sees_the_prior(pkg, orc, gpu):
    """A point seen by one camera has a rank-2 block (the viewing ray is its null space) and fails
    the point rank test alone. The rank test reads V after the fold, so the status is the
    reference's for every prior: a full-rank prior completes the block, and so does the height-only
    prior of ptprior_ref.height, whose one row (z) is not in the span of the observation's two
    (reference pivot ratio 0.018, against 0.25 for the full prior; one more independent row is all a
    rank-2 block needs). A one-row prior along a row of the observation's own Jacobian adds no
    direction and leaves the point deficient."""
    base = cr.bal40(pkg)
    lone = 7
    first = np.flatnonzero(base.obs_point == lone)[0]
    keep = (base.obs_point != lone)
    keep[first] = True
    prob = base.subset(keep).copy()
    assert (prob.obs_point == lone).sum() == 1
    row = orc.eval_jacobians(pkg, prob)[1][np.flatnonzero(prob.obs_point == lone)[0], 0, :3]
    A_in = np.zeros((1, 3, 3))
    A_in[0, 2] = row / np.linalg.norm(row) / 0.01
    one = np.array([lone], np.int32)
    sets = {"none": None, "full": (one, prob.points[[lone]].copy(), (np.eye(3) / 0.01)[None]),
            "height": ppr.height(prob, which=[lone]), "in-span": (one, prob.points[[lone]] + 0.01, A_in)}
    want = {"none": True, "full": False, "height": False, "in-span": True}
    for name, pp in sets.items():
        ref = ppr.covariance(pkg, orc, prob, point_priors=pp)
        c = int(np.flatnonzero(ref["layout"].pt_of == lone)[0])
        g, _ = _cov(pkg, prob.copy(), pp)
        print("one-observation point,", name, "prior: reference ratio", ref["rank"]["point_ratio"][c], "library",
              g["info"]["status"], g["info"]["point_pivot_ratio_min"])
        assert ref["rank"]["deficient"] == want[name], name
        if want[name]:
            assert g["info"]["status"] == "RANK_DEFICIENT" and g["info"]["first_deficient_point"] == lone, name
            assert g["info"]["deficient_points"] == 1
        else:
            assert g["info"]["status"] == "OK", (name, g["info"])
            assert g["info"]["num_residuals"] == 2 * prob.num_obs + 3
            assert g["info"]["point_pivot_ratio_min"] > cr.MIN_PIVOT_RATIO


# ---- 5. two ranks -------------------------------------------------------------------------------
def test_two_ranks_match_single_handle(gpu):
    """The priors split with the shards, at least one on each rank: catches a cost not summed over
    the ranks and a candidate term added after the all-reduce. (A tile bound taken from the local
    cost would not show here: half the cost moves the exponent by one at most. The single-handle
    noise0 case guards the bound.)"""
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
           "--pt-priors", "all", "--iters", "6", "--solvers", "explicit,pcg"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]
    assert '"bal_0"' in p.stdout and '"rig_0"' in p.stdout and '"pt_prior_share"' in p.stdout


# ---- 6. dab_eval_point_priors, state, errors, determinism ---------------------------------------
@pytest.mark.parametrize("case,loss", [("B", None), ("R", pr.CAUCHY2)])
def test_eval_point_priors_against_numpy(pkg, orc, gpu, case, loss):
    prob = pr.CASES[case](pkg)
    idx, mu, A = ppr.all_points(prob)
    perm = np.random.default_rng(5).permutation(len(idx))  # not in point order
    idx, mu, A = idx[perm], mu[perm], A[perm]
    mask = np.zeros(prob.points.shape[0], bool)
    mask[idx[:3]] = True                                    # three priors on constant points: ignored
    s = pkg.Solver(0)
    try:
        if loss:
            s.set_loss(LOSS_NAME[loss[0]], loss[1])
        s.set_problem(prob)
        s.set_points_constant(mask)
        s.set_point_priors(idx, mu, A)
        r, cost = s.eval_point_priors()
        want = np.einsum("nij,nj->ni", A, prob.points[idx] - mu)
        want[:3] = 0.0
        want_cost = 0.5 * (want * want).sum()
        print(case, "residual err", np.abs(r - want).max(), "of", np.abs(want).max(), "cost", cost, want_cost)
        assert np.abs(r - want).max() <= 1e-12 * np.abs(want).max()
        assert cost == pytest.approx(want_cost, rel=1e-12)
        assert (r[:3] == 0.0).all()
        raw_r, raw_cost = s.residuals()          # raw observation quantities: no prior in them
        assert raw_cost == pytest.approx(0.5 * (raw_r * raw_r).sum(), rel=1e-12)
        out = s.solve(_opts(pkg, 2))
        # 0.5 sum rho of the observations (never the prior under the loss) + the prior cost
        rho_cost = rr.cost(*(loss or TRIVIAL), orc.eval_residuals(pkg, pr.CASES[case](pkg))[0])
        assert out["initial_cost"] == pytest.approx(rho_cost + want_cost, rel=1e-12)
        assert out["num_residuals"] == 2 * prob.num_obs + 3 * (len(idx) - 3)
        assert s.get_point_priors()[3] == len(idx) - 3
    finally:
        s.close()


def test_point_prior_state_and_errors(pkg, gpu):
    lib = pkg.load_library()
    start = pr.case_b(pkg)
    prob = start.copy()
    idx, mu, A = _first(ppr.all_points(start), np.array([150, 3, 77]))
    idx, mu, A = np.ascontiguousarray(idx), np.ascontiguousarray(mu), np.ascontiguousarray(A)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)

    def raw(s, n, i, m, a):
        return lib.dab_set_point_priors(s.h, n, None if i is None else i.ctypes.data_as(ip),
                                        None if m is None else m.ctypes.data_as(dp),
                                        None if a is None else a.ctypes.data_as(dp))

    def state(s):
        i, m, a, ne = s.get_point_priors()
        return i.tobytes(), m.tobytes(), a.tobytes(), ne

    s = pkg.Solver(0)
    try:
        n = C.c_int32(-1)
        assert raw(s, 3, idx, mu, A) == -4  # DAB_E_STATE before dab_set_problem
        assert lib.dab_get_point_priors(s.h, C.byref(n), None, None, None, None) == -4 and n.value == -1
        assert lib.dab_eval_point_priors(s.h, None, None) == -4
        s.set_problem(prob)
        assert s.get_point_priors()[0].size == 0 and s.get_point_priors()[3] == 0
        s.set_point_priors(idx, mu, A)
        want = state(s)
        assert want == (idx.tobytes(), mu.tobytes(), A.tobytes(), 3)
        bad_idx, dup, neg = idx.copy(), idx.copy(), idx.copy()
        bad_idx[1] = start.points.shape[0]
        dup[2] = dup[0]
        neg[0] = -1
        nan_mu, inf_a = mu.copy(), A.copy()
        nan_mu[2, 1] = np.nan
        inf_a[1, 2, 2] = np.inf
        for name, args in (("count < 0", (-1, idx, mu, A)), ("null index", (3, None, mu, A)),
                           ("null mean", (3, idx, None, A)), ("null sqrt_info", (3, idx, mu, None)),
                           ("index out of range", (3, bad_idx, mu, A)), ("negative index", (3, neg, mu, A)),
                           ("duplicate", (3, dup, mu, A)), ("nan mean", (3, idx, nan_mu, A)),
                           ("inf sqrt_info", (3, idx, mu, inf_a))):
            assert raw(s, *args) == pkg.DAB_E_INVALID, name
            assert pkg.last_error() != ""
            assert state(s) == want, name
        first = s.solve(_opts(pkg, 6))
        assert first["num_residuals"] == 2 * start.num_obs + 9
        solved = (prob.points.copy(), prob.ext.copy())
        # kept by dab_update_parameters, dab_set_loss, both masks and dab_set_ext_priors
        s.update_parameters(start.points, start.ext)
        s.set_loss("trivial")
        s.set_intrinsics_free(0)
        s.set_points_constant(None)
        s.set_ext_priors(None)
        assert state(s) == want
        again = s.solve(_opts(pkg, 6))            # determinism: two solves are bitwise equal
        assert costs(again) == costs(first) and records(again) == records(first)
        assert [i["gradient_max_norm"] for i in again["iterations"]] == [i["gradient_max_norm"] for i in first["iterations"]]
        np.testing.assert_array_equal(prob.points, solved[0])
        np.testing.assert_array_equal(prob.ext, solved[1])
        # a constant mask over a prior's point takes it out, and lifting the mask brings it back
        m = np.zeros(start.points.shape[0], bool)
        m[idx[0]] = True
        s.set_points_constant(m)
        assert s.get_point_priors()[3] == 2
        s.update_parameters(start.points, start.ext)
        assert s.solve(_opts(pkg, 1))["num_residuals"] == 2 * start.num_obs + 6
        s.set_points_constant(None)
        s.update_parameters(start.points, start.ext)
        assert costs(s.solve(_opts(pkg, 6))) == costs(first)
        # reset by dab_set_problem
        p2 = start.copy()
        s.set_problem(p2)
        assert s.get_point_priors()[0].size == 0 and s.get_point_priors()[3] == 0
        free = s.solve(_opts(pkg, 6))
        assert free["num_residuals"] == 2 * start.num_obs and costs(free) != costs(first)
    finally:
        s.close()
    # a fresh handle walks the same path bitwise, and core.solve's argument is the Solver's
    a = start.copy()
    ra = pkg.solve(a, max_iteration=6, point_priors=(idx, mu, A), num_threads=4)
    assert costs(ra) == costs(first)
    np.testing.assert_array_equal(a.points, solved[0])
    np.testing.assert_array_equal(a.ext, solved[1])


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
    base = cr.bal40(pkg)
    drop = 11
    base = base.subset(base.obs_point != drop).copy()      # point 11 is referenced by no observation
    allp = ppr.all_points(base)
    plain_p = base.copy()
    plain, plain_cov = _run(pkg, plain_p, lambda s: None)
    assert plain_cov["info"]["status"] == "OK"
    mask = np.zeros(base.points.shape[0], bool)
    mask[[4, 9]] = True
    named = (np.array([9, drop, 4], np.int32), base.points[[9, drop, 4]] + 0.5, np.repeat(np.eye(3)[None] * 40.0, 3, axis=0))

    def unreferenced_only(s):
        s.set_point_priors(named[0][1:2], named[1][1:2], named[2][1:2])
        assert s.get_point_priors()[3] == 0

    def set_then_clear(s):
        s.set_point_priors(*allp)
        assert s.get_point_priors()[3] == len(allp[0]) == 199
        s.set_point_priors(None)
        assert s.get_point_priors()[0].size == 0

    def solve_then_clear(s):
        s.set_point_priors(*allp)
        first = s.solve(_opts(pkg, 3))
        assert first["num_residuals"] == 2 * base.num_obs + 3 * 199
        s.update_parameters(base.points, base.ext)
        s.set_point_priors(np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3, 3)))

    for name, setup in (("count 0", lambda s: s.set_point_priors(None)), ("unreferenced only", unreferenced_only),
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

    # constant and unreferenced points named, beside the same mask without any prior
    def masked(s):
        s.set_points_constant(mask)

    def masked_named(s):
        s.set_points_constant(mask)
        s.set_point_priors(*named)
        assert s.get_point_priors()[3] == 0

    pa, pb = base.copy(), base.copy()
    a, ca = _run(pkg, pa, masked)
    b, cb = _run(pkg, pb, masked_named)
    assert costs(a) == costs(b) and records(a) == records(b) and a["num_residuals"] == b["num_residuals"]
    np.testing.assert_array_equal(pa.points, pb.points)
    np.testing.assert_array_equal(pa.ext, pb.ext)
    for k in COV_KEYS:
        np.testing.assert_array_equal(ca[k], cb[k])


def _same_cov(tag, a, b):
    """Every array and every info field of two covariance results, bitwise (timings aside)."""
    assert a.keys() == b.keys(), tag
    for k, x in a.items():
        y = b[k]
        if isinstance(x, dict):
            assert x.keys() == y.keys(), (tag, k)
            for f in x:
                if not f.endswith("_ms"):
                    assert x[f] == y[f] or (x[f] != x[f] and y[f] != y[f]), (tag, k, f, x[f], y[f])
        elif x is None or y is None:
            assert x is None and y is None, (tag, k)
        else:
            np.testing.assert_array_equal(np.asarray(x), np.asarray(y), err_msg=f"{tag}: {k}")


@pytest.mark.parametrize("case", ["shape_a", "rig3x5-mixed"])
def test_empty_effective_set_with_free_intrinsics_is_the_parent_path_bitwise(pkg, orc, gpu, case):
    """The same with free intrinsics (the bordered system and its z block): the solve's records,
    parameters and intrinsics, and every array and info field of dab_covariance_intrinsics."""
    import cov_intr_ref as czr
    import intr_ref as ir
    if case == "shape_a":
        base, groups = ir.shape_a(pkg, orc), 7
    else:
        base, groups = czr.CASES[case](pkg)
    ref_pts = ppr.referenced(base)
    drop = int(ref_pts[5])
    base = base.subset(base.obs_point != drop).copy()      # one point referenced by no observation
    allp = ppr.all_points(base)
    mask = np.zeros(base.points.shape[0], bool)
    mask[ref_pts[[1, 8]]] = True
    named = (np.array([ref_pts[8], drop, ref_pts[1]], np.int32), base.points[[ref_pts[8], drop, ref_pts[1]]] + 0.5,
             np.repeat(np.eye(3)[None] * 40.0, 3, axis=0))

    def run(setup, with_mask=False):
        p = base.copy()
        s = pkg.Solver(0)
        try:
            s.set_problem(p)
            s.set_intrinsics_free(groups)
            if with_mask:
                s.set_points_constant(mask)
            setup(s, p)
            before = s.covariance(full=True, intrinsics=True)   # at the start
            out = s.solve(_opts(pkg, 6))
            after = s.covariance(full=True, intrinsics=True)    # at the solution, refined intrinsics
            return out, p, before, after
        finally:
            s.close()

    def unreferenced_only(s, p):
        s.set_point_priors(named[0][1:2], named[1][1:2], named[2][1:2])
        assert s.get_point_priors()[3] == 0

    def set_then_clear(s, p):
        s.set_point_priors(*allp)
        assert s.get_point_priors()[3] == len(allp[0]) > 0
        s.set_point_priors(None)

    def solve_then_clear(s, p):
        s.set_point_priors(*allp)
        first = s.solve(_opts(pkg, 3))
        assert first["num_residuals"] == 2 * base.num_obs + 3 * len(allp[0])
        with_priors = s.covariance(full=True, intrinsics=True)
        assert with_priors["info"]["num_residuals"] == 2 * base.num_obs + 3 * len(allp[0])
        p.points[...] = base.points
        p.ext[...] = base.ext
        p.intr[...] = base.intr
        s.update_parameters(base.points, base.ext)
        s.update_intrinsics(base.intr)
        s.set_point_priors(np.zeros(0, np.int32), np.zeros((0, 3)), np.zeros((0, 3, 3)))

    def constant_named(s, p):
        s.set_point_priors(*named)
        assert s.get_point_priors()[3] == 0

    for with_mask, setups in ((False, (("count 0", lambda s, p: s.set_point_priors(None)),
                                       ("unreferenced only", unreferenced_only), ("cleared", set_then_clear),
                                       ("solved, then cleared", solve_then_clear))),
                              (True, (("constant and unreferenced named", constant_named),))):
        plain, plain_p, plain_before, plain_after = run(lambda s, p: None, with_mask)
        assert len(plain["iterations"]) > 2 and np.abs(plain_p.intr - base.intr).max() > 0.0
        if case != "shape_a":
            assert plain_before["info"]["status"] == plain_after["info"]["status"] == "OK"
        for name, setup in setups:
            out, p, before, after = run(setup, with_mask)
            tag = f"{case}/{name}"
            assert costs(out) == costs(plain) and records(out) == records(plain), tag
            for k in ("num_parameters", "num_residuals", "schur_assembly", "termination", "final_cost", "initial_cost"):
                assert out[k] == plain[k], (tag, k)
            np.testing.assert_array_equal(p.points, plain_p.points)
            np.testing.assert_array_equal(p.ext, plain_p.ext)
            np.testing.assert_array_equal(p.intr, plain_p.intr)
            _same_cov(tag + "/start", before, plain_before)
            _same_cov(tag + "/solution", after, plain_after)


# ---- 7. the Python host -------------------------------------------------------------------------
def test_solve_point_priors_argument_after_freeze_points(pkg, gpu):
    start = pr.case_b(pkg)
    pp = ppr.all_points(start)
    m = pr.every_third(start)
    a, b = start.copy(), start.copy()
    ra = pkg.solve(a, max_iteration=6, freeze_points=m, point_priors=pp, num_threads=4)
    rb = gpu_solve(pkg, b, pp, const=m, iters=6)
    assert costs(ra) == costs(rb) and ra["num_residuals"] == rb["num_residuals"]
    assert ra["num_residuals"] == 2 * start.num_obs + 3 * int((~m).sum())
    np.testing.assert_array_equal(a.points, b.points)
    sig = pkg.point_sqrt_info_from_sigmas((np.inf, np.inf, 0.01), n=2)
    hz = ppr.height(start, which=[1, 2])
    np.testing.assert_allclose(sig, hz[2], rtol=1e-15)


# ---- 8. the C++ host ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rig", "bal"])
def test_dam_set_point_priors(pkg, orc, gpu, kind):
    import importlib

    import deeparc_ref
    from golden_util import GOLDEN
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_%s.deeparc" % kind)
    prob = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    pp = ppr.all_points(prob)
    n0 = len(pp[0])
    m = host.DeepArcManager()
    m.read(path)
    m.set_point_priors(*pp)
    g = host.solve(m, max_iteration=10)
    p = pkg.solve(prob, max_iteration=10, point_priors=pp)
    plain = pkg.solve(deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path)), max_iteration=10)
    assert g["num_residuals"] == p["num_residuals"] == 2 * prob.num_obs + 3 * n0
    assert records(g) == records(p) and g["termination"] == p["termination"]
    np.testing.assert_allclose(costs(g), costs(p), rtol=1e-9, atol=0)
    assert abs(p["final_cost"] - plain["final_cost"]) > 1e-6 * plain["final_cost"]
    xyz, _ = m.points()
    np.testing.assert_allclose(xyz, prob.points, rtol=0, atol=1e-7)
    # a filter round between two solves (filterPoint3d drops the observations above the bound: the
    # median keeps about half, and the points that lose every observation go with them): the
    # survivors' priors still act under their new indices, the removed points' priors are gone
    r = orc.eval_residuals(pkg, prob)[0]
    before = xyz.copy()
    m.filterPoint3d(float(np.median((r * r).sum(axis=1) / 2.0)), [0.0, 0.0, 0.0], 1e12)
    after, _ = m.points()
    nblocks, npts = len(m.blocks()[0]), after.shape[0]
    assert 0 < nblocks < prob.num_obs and 0 < npts < before.shape[0]
    # which old point each survivor was (the filter keeps the order and the coordinates)
    old = np.array([int(np.flatnonzero((before == x).all(axis=1))[0]) for x in after])
    assert (np.diff(old) > 0).all()
    idx, mu, a = m.get_point_priors()
    keep = np.isin(pp[0], old)
    assert len(idx) == keep.sum() == npts < n0
    np.testing.assert_array_equal(old[idx], pp[0][keep])     # renumbered, never another point's
    np.testing.assert_array_equal(mu, pp[1][keep])
    np.testing.assert_array_equal(a, pp[2][keep])
    g2 = host.solve(m, max_iteration=3)
    assert g2["num_residuals"] == 2 * nblocks + 3 * npts
    # out of range: refused, the setting stays; then cleared
    with pytest.raises(RuntimeError):
        m.set_point_priors(np.array([npts], np.int32), np.zeros((1, 3)), np.eye(3)[None])
    assert host.solve(m, max_iteration=1)["num_residuals"] == 2 * nblocks + 3 * npts
    m.set_point_priors(None)
    assert host.solve(m, max_iteration=1)["num_residuals"] == 2 * nblocks
