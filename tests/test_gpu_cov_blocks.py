"""dab_covariance_blocks on the GPU: the blocks of Sigma = (J^T J)^-1 between a point and another
point, an extrinsic or an intrinsic, folded from C = S^-1 (C' with free intrinsics) and the
per-point records by k_covx_pp / k_covx_pc, against the slices of the dense Sigma
(tests/cov_blocks_ref.py, pinned by tests/test_cov_blocks_ref.py).

Accuracy bound, every returned block: |Sigma_gpu - Sigma_ref| <= 64 kappa 2^-53 m, kappa the
condition number of the (extended) Jacobi-scaled H and m = max |Sigma_ref| over the reference's
full Sigma: the bound of tests/test_gpu_covariance.py and tests/test_gpu_cov_intrinsics.py. Each
case prints the achieved fraction of that bound. Entries known exactly must be +0 bitwise, blocks
without information NaN (cov_blocks_ref.compare).

Cases: tests/cov_blocks_cases.py. Launch geometry: 1, 63, 64, 65 and 257 pairs per list (one
work-group of 64 pairs, its edges, several), one list empty beside the others, every observation's
(point, extrinsic) pair of bal40 and all pairs of 30 points in one call."""
import ctypes as C

import numpy as np
import pytest

import cov_blocks_cases as cases
import cov_blocks_ref as cbr
import cov_ref as cr

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0625
_cache = {}


def ref_of(pkg, orc, name):
    """The reference of a case, computed once and never modified (the solver gets a copy)."""
    if name not in _cache:
        _cache[name] = cases.reference(pkg, orc, name)
    return _cache[name]


def set_env(monkeypatch, sp):
    for k, v in sp["env"].items():
        monkeypatch.setenv(k, v)  # read when the handle is created


def plain_cov(s, sp):
    """The handle's covariance by the existing call of its kind."""
    if np.any(sp["groups"]):
        return s.covariance(full=True, intrinsics=True)
    return s.covariance(full=True)


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("pp", "pe", "pz"))


# ---- accuracy and the properties of one call, per case ---------------------------------------------
@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_accuracy_and_properties(pkg, orc, gpu, name, monkeypatch):
    ref = ref_of(pkg, orc, name)
    sp = ref["spec"]
    set_env(monkeypatch, sp)
    pp, pe, pz = cbr.pair_lists(sp["prob"], 7)
    want, exact = cbr.slices(ref, pp, pe, pz)
    s = cases.solver(pkg, sp)
    try:
        before = plain_cov(s, sp)
        g = s.covariance_blocks(pp=pp, pe=pe, pz=pz)
        g2 = s.covariance_blocks(pp=pp, pe=pe, pz=pz)
        after = plain_cov(s, sp)
    finally:
        s.close()
    assert g["info"]["status"] == "OK", g["info"]
    frac = cbr.compare(g, want, exact, ref["bound"])
    print(f"{name}: largest block error {frac:.3g} of the bound {ref['bound']:.3e} (kappa {ref['kappa']:.3g}, "
          f"m {ref['m']:.3g}), blocks_ms {g['info']['blocks_ms']:.3f}, points_ms {g['info']['points_ms']:.3f}")
    assert same(g, g2)                                             # two calls, bitwise
    for k in before:                                               # the existing call is untouched by the new one
        if isinstance(before[k], np.ndarray):
            assert np.array_equal(before[k], after[k], equal_nan=True), k
    for k in ("num_free_ext", "num_free_points", "num_residuals", "num_parameters", "cost", "schur_assembly"):
        assert g["info"][k] == before["info"][k], k
    # (a, b) beside (b, a): one computation, transposed; a duplicate is the same block
    n = 24
    for i in range(4):
        assert np.array_equal(g["pp"][n + i], g["pp"][i].T, equal_nan=True)
    assert np.array_equal(g["pp"][n + 4:n + 6], g["pp"][:2], equal_nan=True)
    # (a, a) against point_cov: within the bound
    pc = before["point_cov"]
    for i in list(range(n + 6, n + 10)) + [n + 10]:
        a = pp[i, 0]
        assert pp[i, 1] == a
        if np.isnan(pc[a]).any():
            assert np.isnan(g["pp"][i]).all()
        else:
            assert np.abs(g["pp"][i] - pc[a]).max() <= ref["bound"]
    if name == "freeze":
        assert (g["pe"] == 0.0).all() and not np.signbit(g["pe"]).any() and g["info"]["num_free_ext"] == 0
        off = pp[:, 0] != pp[:, 1]
        assert (g["pp"][off] == 0.0).all()
    if name == "bal40-ragged":
        assert np.isnan(g["pp"][-1]).all() and np.isnan(g["pe"][-2]).all()   # point 0 is unreferenced
    if name == "rig6x20-mixed-masks":
        z = pz[:, 1]
        assert (g["pz"][np.isin(z, (1, 4))] == 0.0).all()              # intrinsics outside the free set
        assert exact["pz"][z == 2].any() and not exact["pz"][z == 2].all()


# ---- launch geometry ----------------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_pair_counts(pkg, orc, gpu, count):
    ref = ref_of(pkg, orc, "rig6x20-mixed-g7")
    sp = ref["spec"]
    pp, pe, pz = (x[:count] for x in cbr.pair_lists(sp["prob"], 100 + count, count, count, count))
    assert len(pp) == len(pe) == len(pz) == count
    want, exact = cbr.slices(ref, pp, pe, pz)
    s = cases.solver(pkg, sp)
    try:
        g = s.covariance_blocks(pp=pp, pe=pe, pz=pz)
        # one list empty (not given, or given with no pair) while the others are not
        h1 = s.covariance_blocks(pe=pe, pz=pz)
        h2 = s.covariance_blocks(pp=pp, pe=np.zeros((0, 2), np.int32), pz=pz)
        h3 = s.covariance_blocks(pp=pp)
    finally:
        s.close()
    frac = cbr.compare(g, want, exact, ref["bound"])
    print(f"{count} pairs per list: {frac:.3g} of the bound")
    assert h1["pp"] is None and np.array_equal(h1["pe"], g["pe"]) and np.array_equal(h1["pz"], g["pz"])
    assert h2["pe"].shape == (0, 3, 6) and np.array_equal(h2["pp"], g["pp"]) and np.array_equal(h2["pz"], g["pz"])
    assert h3["pe"] is None and h3["pz"] is None and np.array_equal(h3["pp"], g["pp"])


def test_every_observation_and_all_pairs_of_30_points(pkg, orc, gpu):
    """bal40: the (point, extrinsic) pair of every observation (1600, constant cameras included)
    and all 900 ordered pairs of the first 30 points, in one call."""
    ref = ref_of(pkg, orc, "bal40")
    sp = ref["spec"]
    prob = sp["prob"]
    pe = np.stack([prob.obs_point, prob.obs_ext0], axis=1).astype(np.int32)
    a, b = np.meshgrid(np.arange(30), np.arange(30), indexing="ij")
    pp = np.stack([a.ravel(), b.ravel()], axis=1).astype(np.int32)
    want, exact = cbr.slices(ref, pp, pe)
    s = cases.solver(pkg, sp)
    try:
        g = s.covariance_blocks(pp=pp, pe=pe)
    finally:
        s.close()
    frac = cbr.compare(dict(g, pz=np.zeros((0, 3, 6))), want, exact, ref["bound"])
    print(f"bal40, {len(pe)} pe and {len(pp)} pp pairs: {frac:.3g} of the bound, blocks_ms "
          f"{g['info']['blocks_ms']:.3f}, points_ms {g['info']['points_ms']:.3f}")
    full = g["pp"].reshape(30, 30, 3, 3)
    assert np.array_equal(full, full.transpose(1, 0, 3, 2))     # bitwise: Sigma_ba = Sigma_ab^T
    assert exact["pe"].all(axis=(1, 2)).sum() > 0                # some observations are of constant cameras


# ---- state ------------------------------------------------------------------------------------------------
def _solve5(pkg, sp, with_blocks):
    s = cases.solver(pkg, sp)
    try:
        if with_blocks:
            pp, pe, pz = cbr.pair_lists(sp["prob"], 7)
            assert s.covariance_blocks(pp=pp, pe=pe, pz=pz)["info"]["status"] == "OK"
        out = s.solve(pkg.options(max_num_iterations=5))
        return out, s.problem
    finally:
        s.close()


@pytest.mark.parametrize("name", ["bal40", "rig6x20-mixed-g7"])
def test_solve_after_the_call_is_bitwise_the_same(pkg, orc, gpu, name):
    sp = ref_of(pkg, orc, name)["spec"]
    (sa, a), (sb, b) = _solve5(pkg, sp, False), _solve5(pkg, sp, True)
    keys = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius",
            "success", "valid")
    assert len(sa["iterations"]) == len(sb["iterations"]) >= 3
    for ia, ib in zip(sa["iterations"], sb["iterations"]):
        assert [ia[k] for k in keys] == [ib[k] for k in keys]
    assert (a.points == b.points).all() and (a.ext == b.ext).all() and (a.intr == b.intr).all()


# ---- refusals, fail closed ------------------------------------------------------------------------------
def raw_call(pkg, s, pp=None, pe=None, pz=None, outs=None, with_req=True):
    """dab_covariance_blocks through the bare ABI; outs: the three output arrays or None each.
    Returns (rc, info, zinfo)."""
    req = pkg.DabCovBlocksRequest()
    keep = []
    for name, lst in (("pp", pp), ("pe", pe), ("pz", pz)):
        if lst is None:
            continue
        a = np.ascontiguousarray(np.asarray(lst, np.int32).reshape(-1, 2))
        keep.append(a)
        setattr(req, "num_" + name, a.shape[0])
        setattr(req, name, a.ctypes.data_as(C.POINTER(C.c_int32)))
    outs = outs or [None] * 3
    ptr = [o.ctypes.data_as(C.POINTER(C.c_double)) if o is not None else None for o in outs]
    info, zinfo = pkg.DabCovarianceInfo(), pkg.DabCovarianceIntrInfo()
    rc = s.lib.dab_covariance_blocks(s.h, None, C.byref(req) if with_req else None, *ptr, C.byref(info),
                                     C.byref(zinfo), None)
    return rc, info, zinfo


def sentinels(npp, npe, npz):
    return [np.full((npp, 9), SENTINEL), np.full((npe, 18), SENTINEL), np.full((npz, 18), SENTINEL)]


def test_invalid_requests_write_nothing(pkg, orc, gpu):
    ref = ref_of(pkg, orc, "rig6x20-mixed-g7")
    sp = ref["spec"]
    prob = sp["prob"]
    npts, next_, ni = prob.points.shape[0], prob.ext.shape[0], prob.intr.shape[0]
    good = dict(pp=[(1, 2), (3, 3)], pe=[(1, 2), (4, 0)], pz=[(1, 0), (5, 2)])
    s = cases.solver(pkg, sp)
    try:
        for kind, bad in (("pp", (1, npts)), ("pp", (-1, 2)), ("pe", (npts, 0)), ("pe", (1, next_)), ("pe", (1, -1)),
                          ("pz", (1, ni)), ("pz", (-2, 0))):
            lists = {k: list(v) for k, v in good.items()}
            lists[kind].append(bad)
            outs = sentinels(*(len(lists[k]) for k in ("pp", "pe", "pz")))
            rc, _, _ = raw_call(pkg, s, outs=outs, **lists)
            assert rc == pkg.DAB_E_INVALID and "out of range" in pkg.last_error(), (kind, bad)
            assert all((o == SENTINEL).all() for o in outs)
        # a list without its output array
        outs = sentinels(2, 2, 2)
        rc, _, _ = raw_call(pkg, s, outs=[outs[0], None, outs[2]], **good)
        assert rc == pkg.DAB_E_INVALID and all((o == SENTINEL).all() for o in outs)
        # the size and rank query: no request, or an empty one
        for with_req in (False, True):
            rc, info, zinfo = raw_call(pkg, s, with_req=with_req)
            assert rc == 0 and info.status == 0 and zinfo.num_free_intr == ni
            assert info.num_parameters == ref["layout"].n
        # and the handle still answers
        want, exact = cbr.slices(ref, **good)
        cbr.compare(s.covariance_blocks(**good), want, exact, ref["bound"])
    finally:
        s.close()


def test_rank_deficient_writes_nothing(pkg, gpu):
    prob = cr.DEFICIENT["bal40-gauge"](pkg)
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        outs = sentinels(2, 2, 1)
        rc, info, _ = raw_call(pkg, s, pp=[(1, 2), (3, 3)], pe=[(1, 2), (4, 0)], pz=[(1, 0)], outs=outs)
        assert rc == 0 and info.status == 1 and info.camera_pivot_ratio < 1e-10
        assert all((o == SENTINEL).all() for o in outs)
        g = s.covariance_blocks(pp=[(1, 2)])
        assert g["info"]["status"] == "RANK_DEFICIENT" and g["pp"] is None
    finally:
        s.close()


def test_refusals_of_the_free_set(pkg, gpu):
    """More than 16 free intrinsics, and a free set without a free extrinsic: dab_solve's wording."""
    prob = cr.bal40(pkg)
    g17 = np.zeros(prob.intr.shape[0], np.uint8)
    g17[:17] = 7
    s = pkg.Solver(0)
    try:
        s.set_problem(prob)
        s.set_intrinsics_free(g17)
        outs = sentinels(1, 1, 1)
        rc, _, _ = raw_call(pkg, s, pp=[(1, 2)], pe=[(1, 2)], pz=[(1, 0)], outs=outs)
        assert rc == pkg.DAB_E_UNSUPPORTED and "more than 16 free intrinsics" in pkg.last_error()
        assert all((o == SENTINEL).all() for o in outs)
    finally:
        s.close()
    fixed = prob.copy()
    fixed.ext_const = np.ones(fixed.ext.shape[0], np.uint8)
    s = pkg.Solver(0)
    try:
        s.set_problem(fixed)
        s.set_intrinsics_free(g17 * 0 + np.where(np.arange(len(g17)) < 16, 7, 0).astype(np.uint8))
        outs = sentinels(1, 1, 1)
        rc, _, _ = raw_call(pkg, s, pp=[(1, 2)], pe=[(1, 2)], pz=[(1, 0)], outs=outs)
        assert rc == pkg.DAB_E_UNSUPPORTED and "free intrinsics need a free extrinsic" in pkg.last_error()
        assert all((o == SENTINEL).all() for o in outs)
        s.set_intrinsics_free(None)  # still usable: every camera constant, Sigma_pp' = delta V^-1
        g = s.covariance_blocks(pp=[(1, 1), (1, 2)], pe=[(1, 2)], pz=[(1, 0)])
        assert g["info"]["status"] == "OK" and (g["pe"] == 0.0).all() and (g["pz"] == 0.0).all()
        assert (g["pp"][1] == 0.0).all() and (np.diag(g["pp"][0]) > 0.0).all()
    finally:
        s.close()


# ---- two ranks ------------------------------------------------------------------------------------------
def test_two_ranks_match_single_handle(pkg, orc, gpu):
    """Host-staged, both ranks on one GPU, bal40 with its first 16 intrinsics free, split by point:
    pe and pz blocks of a rank's own points within the bound of the single handle's, a pair naming
    a point of the other rank NaN (scripts/dist_cov_blocks.py)."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tol = cbr.BOUND_FACTOR * ref_of(pkg, orc, "bal40-first16")["kappa"] * cr.EPS
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "scripts", "dist_cov_blocks.py"), "--device", "0", "--tol", repr(tol)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=root)
    print(p.stdout[-1500:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "DIST_COV_BLOCKS OK" in p.stdout, p.stdout[-3000:]
