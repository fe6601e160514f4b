"""dab_covariance_intrinsics on the GPU: Sigma = (J^T J)^-1 over points, free extrinsics and the
active scalars of the free intrinsics, by the exact step's bordered system S' (n' = 6 NC + 6 nfi
rows), its Cholesky factor, the inverse from the factor and the per-point fold-back over cameras
and intrinsics (k_cov_gz), against tests/cov_intr_ref.py (pinned by tests/test_cov_intr_ref.py).

Accuracy bound, every returned array: max |Sigma_gpu - Sigma_ref| <= 64 kappa 2^-53 m, with kappa
the condition number of the Jacobi-scaled H over all columns (intrinsic ones included) and m =
max |Sigma_ref| over all returned blocks: the bound of tests/test_gpu_covariance.py. Each case
prints the achieved fraction of that bound.

Cases (cov_intr_ref.CASES): rig3x5 (n' = 48 < 64, tiles), rig6x20 (points seeing several
intrinsics), the same with mixed models (inactive slots, one focal length driving both rows,
distortion on composed observations) and with per-intrinsic masks (referenced intrinsics that are
not free, a mask that selects no scalar), bal40 / bal170 / bal40-ragged with the first 16 of
their per-camera intrinsics free (16 of 40, a partial last 64-block; pair tables; padding slots
and an unreferenced point), and two focal-only cases."""
import ctypes as C

import numpy as np
import pytest

import cov_intr_ref as czr
import cov_ref as cr
import intr_ref as ir
import lm_ref as lr
import robust_ref as rr

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0625
INFO_FIELDS = ("status", "num_free_ext", "num_free_points", "first_deficient_point", "deficient_points",
               "schur_assembly", "point_pivot_ratio_min", "camera_pivot_ratio", "cost", "num_residuals",
               "num_parameters")

_cache = {}


def case(pkg, orc, name, loss=None):
    """(problem, groups, reference) of a case, computed once and never modified (tests copy)."""
    key = (name, loss)
    if key not in _cache:
        prob, groups = czr.CASES[name](pkg)
        ref = lr.covariance(pkg, orc, prob, groups=groups, loss=czr.LOSSES[loss] if loss else (rr.TRIVIAL, 1.0))
        _cache[key] = (prob, groups, ref)
    return _cache[key]


def gpu_cov(pkg, prob, groups, loss=None, **opts):
    s = pkg.Solver(0)
    try:
        if loss:
            s.set_loss(loss, czr.LOSSES[loss][1])
        s.set_problem(prob)
        s.set_intrinsics_free(groups)
        return s.covariance(full=True, intrinsics=True, **opts)
    finally:
        s.close()


def check_structure(g, ref):
    nfe, nfi = ref["ext_cov"].shape[0], ref["intr_cov"].shape[0]
    full = g["cam_full"]
    assert full.shape == (6 * nfe + 6 * nfi, 6 * nfe + 6 * nfi)
    assert (full == full.T).all()                                                   # bitwise symmetric
    for c in range(nfe):
        assert (full[6 * c:6 * c + 6, 6 * c:6 * c + 6] == g["ext_cov"][c]).all()    # bitwise the same blocks
    o = 6 * nfe
    for i in range(nfi):
        assert (full[o + 6 * i:o + 6 * i + 6, o + 6 * i:o + 6 * i + 6] == g["intr_cov"][i]).all()
    off = np.concatenate([np.zeros(6 * nfe, bool), ~ref["active"].ravel()])
    assert (full[off] == 0.0).all() and (full[:, off] == 0.0).all()                 # known exactly
    assert (np.diag(full)[~off] > 0.0).all()
    for i in range(nfi):
        z = ~ref["active"][i]
        assert (g["intr_cov"][i][z] == 0.0).all() and (g["intr_cov"][i][:, z] == 0.0).all()
    assert (g["ext_index"] == ref["ext_index"]).all()
    assert (g["intr_index"] == ref["intr_index"]).all()
    info, L = g["info"], ref["layout"]
    assert info["num_free_intr"] == nfi and info["num_free_scalars"] == ref["num_free_scalars"]
    assert info["num_parameters"] == 3 * L.np + 6 * L.nc + L.nz == ref["num_parameters"]
    assert info["num_residuals"] == ref["num_residuals"]
    assert info["cost"] == pytest.approx(ref["cost"], rel=1e-12)


def check_accuracy(name, g, ref):
    """Returns the largest error as a fraction of the bound."""
    assert g["info"]["status"] == "OK", g["info"]
    assert g["info"]["camera_pivot_ratio"] > 1e-10
    bound, m = czr.bound(ref)
    nan = np.isnan(ref["point_cov"])
    assert (np.isnan(g["point_cov"]) == nan).all()
    errs = {"point_cov": np.abs(np.where(nan, 0.0, g["point_cov"] - ref["point_cov"])).max()}
    for k in ("ext_cov", "intr_cov", "cam_full"):
        assert g[k].shape == ref[k].shape, k
        errs[k] = np.abs(g[k] - ref[k]).max() if ref[k].size else 0.0
    for k, e in errs.items():
        print(f"{name}: {k} error {e:.3e} = {e / bound:.3g} of the bound {bound:.3e} "
              f"(kappa {ref['kappa']:.3g}, m {m:.3g}, camera + z pivot ratio {g['info']['camera_pivot_ratio']:.3g})")
    for k, e in errs.items():
        assert e <= bound, (k, e, bound)
    check_structure(g, ref)
    return max(errs.values()) / bound


@pytest.mark.parametrize("name", sorted(czr.CASES))
def test_accuracy(pkg, orc, gpu, name):
    prob, groups, ref = case(pkg, orc, name)
    g = gpu_cov(pkg, prob.copy(), groups)
    check_accuracy(name, g, ref)
    nz, n_ext, n_z = czr.SIZES[name]
    assert (g["info"]["num_free_scalars"], 6 * g["info"]["num_free_ext"], 6 * g["info"]["num_free_intr"]) == \
        (nz, n_ext, n_z)
    assert g["info"]["schur_assembly"] == (0 if name.startswith("bal170") else 1)  # pairs | tiles
    if name.startswith("bal40-ragged"):
        assert np.isnan(g["point_cov"][0]).all()


@pytest.mark.parametrize("name,var", [("bal40-first16", "DAB_SCHUR_TILES"), ("rig6x20-mixed", "DAB_INTR_BORDER_LDS")])
def test_assembly_variants(pkg, orc, gpu, name, var, monkeypatch):
    """S by the pair tables where the tiles would serve, and the border sums in global memory."""
    monkeypatch.setenv(var, "0")  # read when the handle is created
    prob, groups, ref = case(pkg, orc, name)
    g = gpu_cov(pkg, prob.copy(), groups)
    check_accuracy(f"{name}/{var}=0", g, ref)
    assert g["info"]["schur_assembly"] == (0 if var == "DAB_SCHUR_TILES" else 1)


@pytest.mark.parametrize("loss", sorted(czr.LOSSES))
def test_accuracy_under_loss(pkg, orc, gpu, loss):
    """Point, camera and intrinsic rows all carry sqrt(rho'), as dab_solve scales them."""
    prob, groups, ref = case(pkg, orc, "rig6x20-mixed", loss)
    g = gpu_cov(pkg, prob.copy(), groups, loss=loss)
    check_accuracy(f"rig6x20-mixed/{loss}", g, ref)
    plain = case(pkg, orc, "rig6x20-mixed")[2]
    assert abs(ref["cost"] - plain["cost"]) > 0.01 * plain["cost"]  # the loss is active on this data


# ---- rank test: fail closed ---------------------------------------------------------------------
def raw_arrays(prob, nfe, nfi):
    n2 = 6 * nfe + 6 * nfi
    return [np.full((prob.points.shape[0], 6), SENTINEL), np.full((nfe, 21), SENTINEL), np.full((nfi, 21), SENTINEL),
            np.full((n2, n2), SENTINEL)]


def raw_call(pkg, s, arrs, opt=None):
    """dab_covariance_intrinsics through the bare ABI. Returns (rc, info, zinfo)."""
    info, zinfo = pkg.DabCovarianceInfo(), pkg.DabCovarianceIntrInfo()
    ptr = [a.ctypes.data_as(C.POINTER(C.c_double)) if a is not None else None for a in arrs]
    rc = s.lib.dab_covariance_intrinsics(s.h, C.byref(opt) if opt is not None else None, *ptr, C.byref(info),
                                         C.byref(zinfo))
    return rc, info, zinfo


@pytest.mark.parametrize("name", ["rig3x5-gauge", "shape_a"])
def test_gauge_free_is_rank_deficient(pkg, orc, gpu, name):
    """Only arc 0 constant: the scale is free, free intrinsics or not."""
    prob = cr.rig3x5(pkg, ()) if name == "rig3x5-gauge" else ir.shape_a(pkg, orc)
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        s.set_intrinsics_free(7)
        rc, info, zinfo = raw_call(pkg, s, [None] * 4)
        assert rc == 0 and info.status == 1 and zinfo.num_free_intr == 3
        arrs = raw_arrays(prob, info.num_free_ext, zinfo.num_free_intr)
        rc, info, zinfo = raw_call(pkg, s, arrs)
    finally:
        s.close()
    print(f"{name}: camera + z pivot ratio {info.camera_pivot_ratio:.3g}")
    assert rc == 0 and info.status == 1
    assert info.deficient_points == 0 and info.first_deficient_point == -1
    assert info.camera_pivot_ratio < 1e-10
    for a in arrs:
        assert (a == SENTINEL).all()


# ---- empty free set: dab_covariance, bitwise ----------------------------------------------------
@pytest.mark.parametrize("name,mask", [("bal40", "never"), ("bal40", "zeros"), ("rig6x20", "never"),
                                       ("rig6x20", "zeros"), ("freeze", "seven")])
def test_empty_free_set_is_dab_covariance(pkg, gpu, name, mask):
    """A mask never set, an all-zero mask, and freeze_camera with every group requested."""
    prob = cr.WELL_POSED[name](pkg)
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        a = s.covariance(full=True)
        if mask != "never":
            s.set_intrinsics_free(np.zeros(prob.intr.shape[0], np.uint8) if mask == "zeros" else 7)
        b = s.covariance(full=True, intrinsics=True)
    finally:
        s.close()
    assert a["info"]["status"] == "OK"
    for k in INFO_FIELDS:
        assert a["info"][k] == b["info"][k] or (np.isnan(a["info"][k]) and np.isnan(b["info"][k])), k
    assert b["info"]["num_free_intr"] == 0 and b["info"]["num_free_scalars"] == 0
    assert b["intr_cov"].shape == (0, 6, 6) and b["intr_index"].shape == (0,)
    for ka, kb in (("point_cov", "point_cov"), ("ext_cov", "ext_cov"), ("ext_full", "cam_full")):
        assert a[ka].shape == b[kb].shape and (a[ka] == b[kb]).all(), kb
    assert (a["ext_index"] == b["ext_index"]).all()


# ---- state ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rig6x20-mixed", "bal40-first16", "bal170-first16"])
def test_two_calls_are_bitwise_equal(pkg, orc, gpu, name):
    prob, groups, _ = case(pkg, orc, name)
    s = pkg.Solver(0)
    try:
        s.set_problem(prob.copy())
        s.set_intrinsics_free(groups)
        a, b = (s.covariance(full=True, intrinsics=True) for _ in range(2))
    finally:
        s.close()
    for k in ("ext_cov", "intr_cov", "cam_full"):
        assert (a[k] == b[k]).all(), k
    assert np.array_equal(a["point_cov"], b["point_cov"], equal_nan=True)


def _solve5(pkg, prob, groups, with_cov):
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        s.set_intrinsics_free(groups)
        if with_cov:
            assert s.covariance(full=True, intrinsics=True)["info"]["status"] == "OK"
            assert (s.get_intrinsics() == prob.intr).all()
            assert (s.get_intrinsics_free()[0] == np.broadcast_to(groups, prob.intr.shape[:1])).all()
            info = pkg.DabCovarianceInfo()  # dab_covariance still refuses this handle
            assert s.lib.dab_covariance(s.h, None, None, None, None, C.byref(info)) == pkg.DAB_E_UNSUPPORTED
            assert "dab_covariance_intrinsics" in pkg.last_error()
        return s.solve(pkg.options(max_num_iterations=5))
    finally:
        s.close()


@pytest.mark.parametrize("name", ["rig6x20-mixed", "bal40-first16", "bal170-first16"])
def test_solve_after_covariance_is_bitwise_the_same(pkg, orc, gpu, name):
    base, groups, _ = case(pkg, orc, name)
    a, b = base.copy(), base.copy()
    sa, sb = _solve5(pkg, a, groups, False), _solve5(pkg, b, groups, True)
    keys = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius",
            "success", "valid")
    assert len(sa["iterations"]) == len(sb["iterations"]) >= 3
    for ia, ib in zip(sa["iterations"], sb["iterations"]):
        assert [ia[k] for k in keys] == [ib[k] for k in keys]
    assert (a.points == b.points).all() and (a.ext == b.ext).all() and (a.intr == b.intr).all()
    assert (a.intr != base.intr).any()  # the solve did refine them


def test_constant_intrinsics_understate_the_variances(pkg, orc, gpu):
    """The reason the call exists: dab_covariance with the mask cleared treats the intrinsics as
    exactly known. On rig6x20 no extrinsic variance of the full answer is smaller, and some exceed
    the intrinsics-constant ones by more than an order of magnitude."""
    prob, groups, _ = case(pkg, orc, "rig6x20")
    s = pkg.Solver(0)
    try:
        s.set_problem(prob.copy())
        s.set_intrinsics_free(groups)
        full = s.covariance(intrinsics=True)
        s.set_intrinsics_free(None)
        const = s.covariance()
    finally:
        s.close()
    ratio = np.diagonal(full["ext_cov"], axis1=1, axis2=2) / np.diagonal(const["ext_cov"], axis1=1, axis2=2)
    print(f"extrinsic variance ratios: {ratio.min():.4g} .. {ratio.max():.4g}")
    assert ratio.min() >= 1.0 and ratio.max() >= 10.0


# ---- refusals and argument errors -----------------------------------------------------------------
def test_refusals_leave_the_handle_usable(pkg, orc, gpu):
    prob, groups, ref = case(pkg, orc, "bal40-first16")
    prob = prob.copy()
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        s.set_intrinsics_free(czr.first(prob, 17))
        arrs = raw_arrays(prob, 38, 17)
        rc, _, _ = raw_call(pkg, s, arrs)
        assert rc == pkg.DAB_E_UNSUPPORTED and "more than 16 free intrinsics" in pkg.last_error()
        for a in arrs:
            assert (a == SENTINEL).all()
        s.set_intrinsics_free(groups)
        check_accuracy("bal40-first16 after a refusal", s.covariance(full=True, intrinsics=True), ref)
    finally:
        s.close()
    fixed = prob.copy()
    fixed.ext_const = np.ones(fixed.ext.shape[0], np.uint8)
    s = pkg.Solver(0)
    try:
        s.set_problem(fixed)
        s.set_intrinsics_free(groups)
        arrs = raw_arrays(fixed, 0, 16)
        rc, _, _ = raw_call(pkg, s, arrs)
        assert rc == pkg.DAB_E_UNSUPPORTED and "free intrinsics need a free extrinsic" in pkg.last_error()
        for a in arrs:
            assert (a == SENTINEL).all()
        s.set_intrinsics_free(None)
        out = s.covariance(intrinsics=True)  # still usable: Sigma_pp = V^-1
        assert out["info"]["status"] == "OK" and out["info"]["num_free_ext"] == 0
    finally:
        s.close()


def test_invalid_arguments(pkg, gpu):
    prob = cr.rig3x5(pkg)
    s = pkg.Solver(0)
    try:
        lib, info, zinfo = s.lib, pkg.DabCovarianceInfo(), pkg.DabCovarianceIntrInfo()
        none = [None] * 4
        assert lib.dab_covariance_intrinsics(s.h, None, *none, C.byref(info), C.byref(zinfo)) == -4  # DAB_E_STATE
        s.set_problem(prob)
        s.set_intrinsics_free(7)
        assert lib.dab_covariance_intrinsics(s.h, None, *none, None, None) == pkg.DAB_E_INVALID
        assert lib.dab_covariance_intrinsics(s.h, None, *none, None, C.byref(zinfo)) == pkg.DAB_E_INVALID
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            o = pkg.covariance_options(min_pivot_ratio=bad)
            assert lib.dab_covariance_intrinsics(s.h, C.byref(o), *none, C.byref(info), None) == pkg.DAB_E_INVALID
        assert lib.dab_covariance_intrinsics(s.h, None, *none, C.byref(info), None) == 0  # zinfo is optional
        assert info.status == 0 and info.num_parameters == 3 * 200 + 30 + 12
    finally:
        s.close()


# ---- two ranks ------------------------------------------------------------------------------------
def test_two_ranks_match_single_handle(pkg, orc, gpu):
    """Host-staged, both ranks on one GPU, bal40 with its first 16 intrinsics free, split by point:
    ext_cov, intr_cov and cam_full bitwise equal across the ranks, and they and every owner's point
    rows within the accuracy bound of the single handle."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tol = 64.0 * case(pkg, orc, "bal40-first16")[2]["kappa"] * cr.EPS
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "scripts", "dist_check.py"), "--device", "0", "--host-collective",
           "--covariance", "--cov-intrinsics", "16", "--iters", "0", "--cov-tol", repr(tol)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    print(p.stdout[-1500:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_CHECK OK" in p.stdout, p.stdout[-3000:]
    assert '"ranks_equal": true' in p.stdout


# ---- host API -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rig", "bal"])
def test_host_manager_covariance_intrinsics(pkg, gpu, kind):
    """DeepArcManager.covarianceIntrinsics on the committed tiny scene with one extra constant
    extrinsic and every group free: bitwise Solver.covariance(intrinsics=True) on the same arrays."""
    import importlib
    import os

    import deeparc_ref
    from golden_util import GOLDEN
    host = importlib.import_module(pkg.__name__ + ".host_api")
    path = os.path.join(GOLDEN, "tiny_%s.deeparc" % kind)
    m = host.DeepArcManager()
    m.read(path)
    m.set_intrinsics_free(7)
    loose = m.covariance_intrinsics()
    assert loose["info"]["status"] == "RANK_DEFICIENT" and loose["point_cov"] is None
    g = m.covariance_intrinsics(extra_const=(1,), full=True)
    assert g["info"]["status"] == "OK"
    prob = deeparc_ref.to_problem(pkg, deeparc_ref.read_deeparc(path))
    prob.ext_const[1] = 1
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        s.set_intrinsics_free(7)
        d = s.covariance(full=True, intrinsics=True)
    finally:
        s.close()
    assert d["info"]["status"] == "OK" and d["info"]["num_free_intr"] == prob.intr.shape[0]
    for k in ("point_cov", "ext_cov", "intr_cov", "cam_full"):
        assert g[k].shape == d[k].shape and (g[k] == d[k]).all(), k
    assert (g["ext_index"] == d["ext_index"]).all() and (g["intr_index"] == d["intr_index"]).all()
    for k in ("num_parameters", "num_residuals", "num_free_scalars", "num_free_intr", "cost"):
        assert g["info"][k] == d["info"][k], k
    m.set_intrinsics_free(0)  # no group: covariance(), cam_full = ext_full
    e, f = m.covariance_intrinsics(extra_const=(1,), full=True), m.covariance(extra_const=(1,), full=True)
    assert e["intr_cov"].shape == (0, 6, 6) and (e["cam_full"] == f["ext_full"]).all()
    assert (e["point_cov"] == f["point_cov"]).all() and (e["ext_cov"] == f["ext_cov"]).all()
