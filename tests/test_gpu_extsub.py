"""Constant scalars of an extrinsic on the GPU (dab_set_ext_scalars_constant): the mask through
dab_solve and both covariances, against tests/extsub_ref.py (pinned by tests/test_extsub_ref.py,
which also measures the reference's own spread on every case: at most 1.2e-12 of the cost and
2e-12 of the parameters).

Tolerances are the project's: same iteration records and termination, initial cost
1e-12, per-iteration cost 1e-9 relative, parameters 1e-7; PCG run to convergence against EXPLICIT
1e-6; covariance blocks 64 kappa 2^-53 max|Sigma|. Constant scalars are compared bit for bit
everywhere."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_ref as cr
import extsub_ref as xr
import lm_ref as lr
import prior_ref as qr
import robust_ref as rr

pytestmark = pytest.mark.gpu

LOSS_NAME = {rr.TRIVIAL: None, rr.CAUCHY: "cauchy"}


def records(s):
    return [(i["success"], i["valid"]) for i in s["iterations"]]


def costs(s):
    return [i["cost"] for i in s["iterations"]]


def _opts(pkg, iters, lst=None, **kw):
    return pkg.options(max_num_iterations=iters, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR if lst is None else lst, **kw)


def held_of(prob, bits):
    """[num_ext][6] bool: the scalars the bits name (effective or not)."""
    return ((xr.as_bits(prob, bits)[:, None] >> np.arange(6)) & 1).astype(bool)


def gpu_solve(pkg, prob, bits, iters=25, loss=None, groups=0, lst=None, const=None, priors=None, **kw):
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
        if bits is not None:
            s.set_ext_scalars_constant(bits)
        return s.solve(_opts(pkg, iters, lst, **kw))
    finally:
        s.close()


_ref = {}


def reference(pkg, orc, key, make, mask, iters, loss=None, **kw):
    """(summary, solved problem, start, bits) of extsub_ref.lm, computed once per key, never modified."""
    if key not in _ref:
        start = make()
        p = start.copy()
        b = xr.MASKS[mask](p) if isinstance(mask, str) else mask
        _ref[key] = (xr.lm(pkg, orc, p, _opts(pkg, iters), bits=b, loss=loss or lr.TRIVIAL, **kw), p, start, b)
    return _ref[key]


def check_against(tag, g, prob, ref, cost_tol=1e-9):
    o, pref, start, b = ref
    err = max((abs(x - y) / abs(y) for x, y in zip(costs(g), costs(o))), default=0.0)
    print(tag, g["termination"], g["num_iterations"], "cost", g["initial_cost"], "->", g["final_cost"], "rejected",
          g["num_unsuccessful_steps"], "assembly", g["schur_assembly"], "max rel cost err", err, "points err",
          np.abs(prob.points - pref.points).max(), "ext err", np.abs(prob.ext - pref.ext).max())
    assert g["termination"] == o["termination"], (g["message"], o["message"])
    assert g["num_iterations"] == o["num_iterations"]
    assert records(g) == records(o)
    assert g["initial_cost"] == pytest.approx(o["initial_cost"], rel=1e-12)
    for x, y in zip(g["iterations"], o["iterations"]):
        assert abs(x["cost"] - y["cost"]) <= cost_tol * abs(y["cost"]), (x, y)
    assert np.abs(prob.points - pref.points).max() < 1e-7
    assert np.abs(prob.ext - pref.ext).max() < 1e-7
    assert (np.abs(prob.intr - pref.intr) <= 1e-7 * np.maximum(1.0, np.abs(pref.intr))).all()
    h = held_of(start, b)
    assert prob.ext[h].tobytes() == start.ext[h].tobytes()  # bitwise untouched (also on constant extrinsics)
    assert g["num_parameters"] == o["num_parameters"] and g["num_free_points"] == o["num_free_points"]
    assert g["num_free_ext"] == o["num_free_ext"]


def traj_ref(pkg, orc, t):
    case, mask, loss, iters = t
    return reference(pkg, orc, ("traj",) + tuple(map(str, t)), lambda: xr.CASES[case](pkg), mask, iters, loss)


# ---- 1. trajectories ----------------------------------------------------------------------------
@pytest.mark.parametrize("t", xr.TRAJECTORIES, ids=xr.traj_id)
def test_trajectory_matches_reference(pkg, orc, gpu, t):
    case, mask, loss, iters = t
    ref = traj_ref(pkg, orc, t)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], iters, loss)
    check_against(xr.traj_id(t), g, prob, ref)
    L = xr.SubLayout(ref[2], None, 0, ref[3])
    assert g["num_parameters"] == 3 * L.np + 6 * L.nc - L.n_sub and L.n_sub > 0
    if (case, mask, loss) in (("Blow", "trans-all", None), ("R", "mix", None)):
        assert g["num_unsuccessful_steps"] > 0  # rejected steps: the constant scalars still never move


def test_negative_zero_is_kept(pkg, orc, gpu):
    start = xr.CASES["Blow"](pkg)
    start.ext[3, 4] = -0.0
    ref = reference(pkg, orc, ("negzero",), lambda: start, "trans-all", 6)
    prob = start.copy()
    g = gpu_solve(pkg, prob, ref[3], 6)
    check_against("Blow/trans-all/-0.0", g, prob, ref)
    assert np.signbit(prob.ext[3, 4]) and prob.ext[3, 4] == 0.0


# ---- 2. both assemblies -------------------------------------------------------------------------
@pytest.mark.parametrize("tiles", ["0", "1"])
@pytest.mark.parametrize("t", [("R", "mix", None, 25), ("Blow", "rot-odd", None, 25)], ids=xr.traj_id)
def test_trajectory_both_assemblies(pkg, orc, gpu, t, tiles, monkeypatch):
    monkeypatch.setenv("DAB_SCHUR_TILES", tiles)  # read when the handle is created
    ref = traj_ref(pkg, orc, t)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], t[3], t[2])
    check_against(f"{xr.traj_id(t)}/tiles={tiles}", g, prob, ref)
    assert g["schur_assembly"] == int(tiles)


# ---- 3. the direct path -------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["Blow", "R"])
def test_direct_path(pkg, orc, gpu, case):
    """All points constant plus mix: per-camera 6x6 solves (Blow), the dense form with cross blocks (R)."""
    ref = reference(pkg, orc, ("direct", case), lambda: xr.CASES[case](pkg), "mix", 15, const=True)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], 15, const=True)
    check_against(f"{case}/mix/all points constant", g, prob, ref)
    assert g["schur_assembly"] == pkg.DAB_SCHUR_DIRECT and g["num_free_points"] == 0
    np.testing.assert_array_equal(prob.points, ref[2].points)


# ---- 4. PCG -------------------------------------------------------------------------------------
def _pcg(pkg, prob, bits, how, monkeypatch, iters=5, **kw):
    if how.startswith("stored-y"):
        monkeypatch.setenv("DAB_PCG_MF", "0")
    return gpu_solve(pkg, prob, bits, iters, lst=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG,
                     pcg_fp32=int(how.endswith("fp32")), **kw)


@pytest.mark.parametrize("how", ["stored-y", "matrix-free", "matrix-free-fp32"])
def test_pcg_converged_matches_explicit(pkg, gpu, how, monkeypatch):
    start = xr.CASES["Blow"](pkg)
    b = xr.trans_all(start)
    pe, pp = start.copy(), start.copy()
    e = gpu_solve(pkg, pe, b, 5)
    p = _pcg(pkg, pp, b, how, monkeypatch, eta=1e-14, max_linear_solver_iterations=1000)
    want = {"stored-y": 0, "matrix-free": 1, "matrix-free-fp32": 2}[how]
    print(how, "explicit", repr(e["final_cost"]), "pcg", repr(p["final_cost"]), "assembly", p["schur_assembly"],
          "max rel", max(abs(x - y) / abs(y) for x, y in zip(costs(p), costs(e))))
    assert p["schur_assembly"] == want
    assert records(e) == records(p)
    np.testing.assert_allclose(costs(p), costs(e), rtol=1e-6, atol=0)
    h = held_of(start, b)
    assert pp.ext[h].tobytes() == start.ext[h].tobytes()
    assert p["num_parameters"] == e["num_parameters"] == 3 * e["num_free_points"] + 3 * e["num_free_ext"]


@pytest.mark.parametrize("how", ["stored-y", "matrix-free"])
def test_pcg_truncated_is_repeatable_bitwise(pkg, gpu, how, monkeypatch):
    start = xr.CASES["R"](pkg)
    b = xr.mix(start)
    pa, pb = start.copy(), start.copy()
    x = _pcg(pkg, pa, b, how, monkeypatch, iters=4, max_linear_solver_iterations=6)
    y = _pcg(pkg, pb, b, how, monkeypatch, iters=4, max_linear_solver_iterations=6)
    assert costs(x) == costs(y) and records(x) == records(y)
    assert pa.ext.tobytes() == pb.ext.tobytes() and pa.points.tobytes() == pb.points.tobytes()
    assert x["final_cost"] < x["initial_cost"]


# ---- 5. free intrinsics -------------------------------------------------------------------------
def test_free_intrinsics(pkg, orc, gpu):
    ref = reference(pkg, orc, ("intr",), lambda: xr.CASES["R"](pkg), "rot-odd", 10, groups=7)
    prob = ref[2].copy()
    g = gpu_solve(pkg, prob, ref[3], 10, groups=7)
    check_against("R/rot-odd/groups 7", g, prob, ref)
    assert g["schur_assembly"] in (pkg.DAB_SCHUR_PAIRS, pkg.DAB_SCHUR_TILES)
    assert np.abs(prob.intr - ref[2].intr).max() > 0.0


# ---- 6. an extrinsic prior on an extrinsic with constant translation ----------------------------
def test_prior_on_constant_translation(pkg, orc, gpu):
    start = xr.CASES["Blow"](pkg)
    priors = qr.pose(start)
    ref = reference(pkg, orc, ("prior",), lambda: start, "trans-all", 10, priors=priors)
    prob = start.copy()
    g = gpu_solve(pkg, prob, ref[3], 10, priors=priors)
    check_against("Blow/trans-all/pose priors", g, prob, ref)
    assert g["num_residuals"] == ref[0]["num_residuals"] == 2 * start.num_obs + 6 * len(priors[0])
    # the offset A_t (t - mu_t) is in the cost: without it the initial cost differs
    free = gpu_solve(pkg, start.copy(), ref[3], 0)
    assert abs(g["initial_cost"] - free["initial_cost"]) > 1e-6 * free["initial_cost"]


# ---- 7. all six bits on one extrinsic -----------------------------------------------------------
@pytest.mark.parametrize("case,e", [("Blow", 5), ("R", 6)])
def test_all_six_bits_agree_with_ext_const(pkg, gpu, case, e):
    pa, pb = xr.CASES[case](pkg), xr.CASES[case](pkg)
    pa.ext_const[e] = 1
    bits = np.zeros(pb.ext.shape[0], np.uint8)
    bits[e] = 63
    a = gpu_solve(pkg, pa, None, 10)
    b = gpu_solve(pkg, pb, bits, 10)
    print(case, e, "max rel", max(abs(x - y) / abs(y) for x, y in zip(costs(a), costs(b))), "ext",
          np.abs(pa.ext - pb.ext).max())
    assert records(a) == records(b) and a["termination"] == b["termination"]
    np.testing.assert_allclose(costs(b), costs(a), rtol=1e-9, atol=0)
    assert np.abs(pa.ext - pb.ext).max() < 1e-7 and np.abs(pa.points - pb.points).max() < 1e-7
    assert b["num_free_ext"] == a["num_free_ext"] + 1 and b["num_parameters"] == a["num_parameters"]


# ---- 8. no free parameter -----------------------------------------------------------------------
@pytest.mark.parametrize("lst", ["explicit", "pcg", "auto"])
def test_no_free_parameter(pkg, orc, gpu, lst):
    start = xr.CASES["Blow"](pkg)
    prob = start.copy()
    which = {"explicit": pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, "pcg": pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG,
             "auto": pkg.DAB_LINEAR_SOLVER_AUTO}[lst]
    g = gpu_solve(pkg, prob, 63, 25, lst=which, const=True)
    o = xr.lm(pkg, orc, start.copy(), _opts(pkg, 25), bits=63, const=True)
    assert (g["termination"], g["num_iterations"], g["iterations"]) == ("CONVERGENCE", 0, [])
    assert g["message"] == o["message"] == lr.NO_FREE_MESSAGE
    assert g["initial_cost"] == g["final_cost"] == pytest.approx(o["initial_cost"], rel=1e-12)
    assert (g["num_parameters"], g["num_free_points"], g["num_free_ext"]) == (0, 0, o["num_free_ext"])
    assert prob.points.tobytes() == start.points.tobytes() and prob.ext.tobytes() == start.ext.tobytes()


# ---- 9. an empty effective mask -----------------------------------------------------------------
def _run(pkg, prob, setup, iters=6, groups=None):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        if groups is not None:
            s.set_intrinsics_free(groups)
        setup(s)
        out = s.solve(_opts(pkg, iters))
        cov = s.covariance(full=True, intrinsics=groups is not None)
        return out, cov
    finally:
        s.close()


def _same(out, cov, p, plain, plain_cov, plain_p, name):
    assert costs(out) == costs(plain) and records(out) == records(plain), name
    for k in ("num_parameters", "num_free_ext", "schur_assembly", "termination", "final_cost"):
        assert out[k] == plain[k], (name, k)
    assert p.points.tobytes() == plain_p.points.tobytes() and p.ext.tobytes() == plain_p.ext.tobytes(), name
    assert cov["info"]["status"] == plain_cov["info"]["status"] == "OK"
    for k in ("point_cov", "ext_cov", "ext_full", "cam_full", "intr_cov"):
        if k in plain_cov:
            np.testing.assert_array_equal(cov[k], plain_cov[k], err_msg=name)
    assert cov["info"]["num_parameters"] == plain_cov["info"]["num_parameters"]


def test_empty_effective_mask_is_the_parent_path_bitwise(pkg, gpu):
    base = cr.bal40(pkg)  # cameras 0 and 1 constant
    base = base.subset(base.obs_ext0 != 9).copy()  # extrinsic 9 is referenced by no observation
    ne = base.ext.shape[0]
    only_ignored = np.zeros(ne, np.uint8)
    only_ignored[[0, 1, 9]] = [63, 56, 7]
    plain_p = base.copy()
    plain, plain_cov = _run(pkg, plain_p, lambda s: None)

    def set_then_clear(s):
        s.set_ext_scalars_constant(56)
        assert s.get_ext_scalars_constant()[1] == 3 * (ne - 3)
        s.set_ext_scalars_constant(None)

    def ignored(s):
        s.set_ext_scalars_constant(only_ignored)
        got, n = s.get_ext_scalars_constant()
        assert (got == only_ignored).all() and n == 0

    for name, setup in (("null", lambda s: s.set_ext_scalars_constant(None)),
                        ("zeros", lambda s: s.set_ext_scalars_constant(np.zeros(ne, np.uint8))),
                        ("ignored", ignored), ("cleared", set_then_clear)):
        p = base.copy()
        out, cov = _run(pkg, p, setup)
        _same(out, cov, p, plain, plain_cov, plain_p, name)
    # freeze_camera: no extrinsic is free, every bit is ignored
    fz = base.copy()
    fz.freeze_camera = True
    fa, fb = fz.copy(), fz.copy()
    pa, ca = _run(pkg, fa, lambda s: None)

    def frozen(s):
        s.set_ext_scalars_constant(63)
        assert s.get_ext_scalars_constant()[1] == 0

    pb, cb = _run(pkg, fb, frozen)
    _same(pb, cb, fb, pa, ca, fa, "freeze_camera")
    # and through dab_covariance_intrinsics
    rig = cr.rig6x20(pkg)
    ra, rb = rig.copy(), rig.copy()
    qa, za = _run(pkg, ra, lambda s: None, 3, 7)
    bits = np.zeros(rig.ext.shape[0], np.uint8)
    bits[np.flatnonzero(rig.ext_const)] = 63
    qb, zb = _run(pkg, rb, lambda s: s.set_ext_scalars_constant(bits), 3, 7)
    _same(qb, zb, rb, qa, za, ra, "intrinsics")


# ---- 10. state and errors -----------------------------------------------------------------------
def test_mask_state_and_errors(pkg, gpu):
    lib = pkg.load_library()
    start = xr.CASES["Blow"](pkg)
    ne = start.ext.shape[0]
    prob = start.copy()
    b = xr.mix(start)
    eff = int(sum(bin(int(x)).count("1") for e, x in enumerate(b) if not start.ext_const[e]))
    u8 = C.POINTER(C.c_uint8)
    s = pkg.Solver(0)
    try:
        buf = (C.c_uint8 * ne)()
        n = C.c_int32(-1)
        assert lib.dab_set_ext_scalars_constant(s.h, buf) == -4  # DAB_E_STATE before dab_set_problem
        assert lib.dab_get_ext_scalars_constant(s.h, buf, C.byref(n)) == -4
        assert lib.dab_set_ext_scalars_constant(None, buf) == pkg.DAB_E_INVALID
        s.set_problem(prob)
        assert s.get_ext_scalars_constant()[1] == 0 and not s.get_ext_scalars_constant()[0].any()
        s.set_ext_scalars_constant(b)
        got, cnt = s.get_ext_scalars_constant()
        assert (got == b).all() and cnt == eff
        assert lib.dab_get_ext_scalars_constant(s.h, None, None) == 0
        # a byte of 64: refused, the state stays
        bad = b.copy()
        bad[2] = 64
        assert lib.dab_set_ext_scalars_constant(s.h, bad.ctypes.data_as(u8)) == pkg.DAB_E_INVALID
        got, cnt = s.get_ext_scalars_constant()
        assert (got == b).all() and cnt == eff
        first = s.solve(_opts(pkg, 6))
        assert first["num_parameters"] == 3 * first["num_free_points"] + 6 * first["num_free_ext"] - eff
        solved = prob.ext.copy()
        # kept by every other setter: the same start walks the same path
        s.update_parameters(start.points, start.ext)
        s.set_loss("trivial")
        s.set_points_constant(None)
        s.set_intrinsics_free(None)
        s.set_ext_priors(None)
        s.set_point_priors(None)
        assert s.get_ext_scalars_constant()[1] == eff
        again = s.solve(_opts(pkg, 6))
        assert costs(again) == costs(first)
        assert prob.ext.tobytes() == solved.tobytes()
        h = held_of(start, b)
        pts, ext = np.zeros_like(start.points), np.zeros_like(start.ext)
        s.get_parameters(pts, ext)
        assert ext[h].tobytes() == start.ext[h].tobytes()
        # reset by dab_set_problem
        p2 = start.copy()
        s.set_problem(p2)
        assert s.get_ext_scalars_constant()[1] == 0 and not s.get_ext_scalars_constant()[0].any()
        free = s.solve(_opts(pkg, 6))
        assert free["num_parameters"] == first["num_parameters"] + eff
        assert np.abs(p2.ext[h] - start.ext[h]).max() > 1e-6
    finally:
        s.close()
    # core.solve's switch is the Solver's
    a = start.copy()
    ra = pkg.solve(a, max_iteration=6, ext_scalars_constant=b, num_threads=4)
    assert costs(ra) == costs(first) and a.ext.tobytes() == solved.tobytes()


# ---- 11. gauge ----------------------------------------------------------------------------------
def _cov(pkg, prob, bits, groups=None):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        if groups is not None:
            s.set_intrinsics_free(groups)
        if bits is not None:
            s.set_ext_scalars_constant(bits)
        return s.covariance(full=True, intrinsics=groups is not None)
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
    assert g["info"]["num_parameters"] == ref["num_parameters"]
    assert g["info"]["num_free_ext"] == ref["layout"].nc
    assert g["info"]["cost"] == pytest.approx(ref["cost"], rel=1e-12)
    full = g[full_key]
    assert full.tobytes() == np.ascontiguousarray(full.T).tobytes()  # bitwise symmetric
    held = np.flatnonzero(~ref["ext_free"].ravel())
    assert len(held) > 0
    assert not full[held].any() and not full[:, held].any()  # exactly 0 (known exactly)
    assert not np.signbit(full[held]).any()
    for c in range(g["ext_cov"].shape[0]):
        assert (full[6 * c:6 * c + 6, 6 * c:6 * c + 6] == g["ext_cov"][c]).all()
    rest = np.setdiff1d(np.arange(6 * g["ext_cov"].shape[0]), held)
    assert (np.diag(full)[rest] > 0.0).all()


@pytest.mark.parametrize("name", sorted(xr.GAUGE))
def test_one_translation_scalar_fixes_the_gauge(pkg, orc, gpu, name):
    make, e, k = xr.GAUGE[name]
    prob = make(pkg)
    free = _cov(pkg, prob.copy(), None)
    rot = _cov(pkg, prob.copy(), xr.one_bit(prob, e, 0))
    for g in (free, rot):
        assert g["info"]["status"] == "RANK_DEFICIENT" and g["point_cov"] is None
    assert rot["info"]["num_parameters"] == free["info"]["num_parameters"] - 1
    bits = xr.one_bit(prob, e, k)
    ref = xr.covariance(pkg, orc, prob, bits=bits)
    assert not ref["rank"]["deficient"]
    g = _cov(pkg, prob.copy(), bits)
    _check_cov(f"{name}/bit {k} of extrinsic {e}", g, ref, "ext_full")
    assert g["info"]["camera_pivot_ratio"] > 1e-3


def test_gauge_through_covariance_intrinsics(pkg, orc, gpu):
    """Deficient without the bit, DAB_COV_OK and within the covariance bound with it. The camera
    pivot ratio is not asserted above 1e-3 here: with groups 7 free the reference's own ratio is
    2.8e-6 (kappa 8.7e8), set by the intrinsic columns and not by the gauge; it must pass the
    call's own threshold, 1e-10 (measured on the GPU: 2.79e-6)."""
    make, e, k = xr.GAUGE["rig6x20"]
    prob = make(pkg)
    bits = xr.one_bit(prob, e, k)
    assert _cov(pkg, prob.copy(), None, 7)["info"]["status"] == "RANK_DEFICIENT"
    ref = xr.covariance(pkg, orc, prob, bits=bits, groups=7)
    assert not ref["rank"]["deficient"]
    g = _cov(pkg, prob.copy(), bits, 7)
    _check_cov("rig6x20/groups 7/bit 4", g, ref, "cam_full")
    assert g["info"]["num_free_scalars"] == ref["num_free_scalars"] > 0
    assert g["info"]["camera_pivot_ratio"] > 1e-10


# ---- 12. two ranks ------------------------------------------------------------------------------
def test_two_ranks_match_single_handle(gpu):
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
           "--ext-scalars", "mix", "--iters", "6", "--solvers", "explicit,pcg"]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]
    assert '"bal_0"' in p.stdout and '"rig_0"' in p.stdout and '"const_held": true' in p.stdout


# ---- 13. the C++ host ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rig", "bal"])
def test_dam_set_ext_scalars_constant(pkg, gpu, kind):
    import importlib

    import deeparc_ref
    from golden_util import GOLDEN
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_%s.deeparc" % kind)
    prob = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    bits = xr.mix(prob)
    m = host.DeepArcManager()
    m.read(path)
    cams0 = m.cameras()[0].copy()
    m.set_ext_scalars_constant(bits)
    g = host.solve(m, max_iteration=10)
    p = pkg.solve(prob, max_iteration=10, ext_scalars_constant=bits)
    plain = pkg.solve(deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path)), max_iteration=10)
    assert g["num_parameters"] == p["num_parameters"] < plain["num_parameters"]
    assert records(g) == records(p) and g["termination"] == p["termination"]
    np.testing.assert_allclose(costs(g), costs(p), rtol=1e-9, atol=0)
    cams = m.cameras()[0]
    np.testing.assert_allclose(cams, prob.ext, rtol=0, atol=1e-7)
    h = held_of(prob, bits)
    assert cams[h].tobytes() == cams0[h].tobytes() and np.abs(cams - cams0).max() > 0.0
    # kept across a re-set of the resident problem (freeze_camera changes the constancy), then back
    z = host.solve(m, max_iteration=2, freeze_camera=True)
    assert z["num_free_ext"] == 0
    again = host.solve(m, max_iteration=1)
    assert again["num_parameters"] == g["num_parameters"]
    # a byte above 63: refused, the setting stays; then cleared
    bad = bits.copy()
    bad[0] = 64
    with pytest.raises(RuntimeError):
        m.set_ext_scalars_constant(bad)
    assert host.solve(m, max_iteration=1)["num_parameters"] == g["num_parameters"]
    m.set_ext_scalars_constant(None)
    assert host.solve(m, max_iteration=1)["num_parameters"] == plain["num_parameters"]
