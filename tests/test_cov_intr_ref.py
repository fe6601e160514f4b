"""CPU tests of the reference of dab_covariance_intrinsics (tests/cov_intr_ref.py) and of the part
of the call's C ABI that needs no device. The GPU tests (test_gpu_cov_intrinsics.py) trust the
reference only because these pin it: the inverse of the Jacobi-scaled normal matrix over points,
extrinsics and active intrinsic scalars against the SVD pseudo-inverse of the same Jacobian,
within the bound the GPU tests use (64 kappa 2^-53 max |Sigma|), the sizes of every shared case,
and the rank test on the well-posed and the gauge-free shapes."""
import ctypes as C

import numpy as np
import pytest

import cov_intr_ref as czr
import cov_ref as cr
import intr_ref as ir
import lm_ref as lr
import robust_ref as rr

LOSSY = [("rig6x20-mixed", "huber"), ("rig6x20-mixed", "cauchy")]


@pytest.fixture(scope="module")
def jac(pkg, orc):
    cache = {}

    def get(name, loss=None):
        if (name, loss) not in cache:
            prob, groups = czr.CASES[name](pkg)
            cache[(name, loss)] = (prob, groups) + lr.jacobian(pkg, orc, prob, groups=groups,
                                                               loss=czr.LOSSES[loss] if loss else (rr.TRIVIAL, 1.0))
        return cache[(name, loss)]
    return get


@pytest.mark.parametrize("name,loss", [(n, None) for n in sorted(czr.CASES)] + LOSSY)
def test_two_routes_agree(jac, name, loss):
    """inv of the scaled H, unscaled, against pinv(J) pinv(J)^T, within the GPU tests' bound."""
    prob, groups, L, A, _ = jac(name, loss)
    a, b = cr.sigma_inv(A), cr.sigma_pinv(A)
    kappa = cr.kappa(A)
    bound = 64.0 * kappa * cr.EPS * np.abs(b).max()
    err = np.abs(a - b).max()
    print(f"{name} {loss}: n = {L.n}, nz = {L.nz}, kappa = {kappa:.3g}, routes differ by {err:.2e} = "
          f"{err / bound:.3g} of the bound, relative {err / np.abs(b).max():.2e}")
    assert err <= bound
    assert L.n == A.shape[1] and A.shape[0] == 2 * prob.num_obs


@pytest.mark.parametrize("name", sorted(czr.CASES))
def test_sizes_and_blocks(jac, name):
    prob, groups, L, A, _ = jac(name)
    nz, n_ext, n_z = czr.SIZES[name]
    assert (L.nz, 6 * L.nc, 6 * len(czr.free_intrinsics(L))) == (nz, n_ext, n_z)
    rng = np.random.default_rng(1)
    M = rng.normal(size=(L.n, L.n))
    Sigma = M @ M.T  # any symmetric matrix: the split is bookkeeping
    b = czr.blocks(Sigma, L, prob)
    full, act = b["cam_full"], b["active"]
    assert full.shape == (n_ext + n_z, n_ext + n_z) and (full == full.T).all()
    assert act.sum() == nz and b["intr_cov"].shape == (n_z // 6, 6, 6)
    off = np.concatenate([np.zeros(n_ext, bool), ~act.ravel()])
    assert (full[off] == 0.0).all() and (full[:, off] == 0.0).all()
    assert (full[~off][:, ~off] == Sigma[3 * L.np:, 3 * L.np:]).all()  # (index, slot) order both ways
    for i in range(n_z // 6):
        o = n_ext + 6 * i
        assert (b["intr_cov"][i] == full[o:o + 6, o:o + 6]).all()


@pytest.mark.parametrize("name,loss", [(n, None) for n in sorted(czr.CASES)] + LOSSY)
def test_rank_test_passes_well_posed(jac, name, loss):
    _, _, L, A, _ = jac(name, loss)
    t = czr.rank_test(A, L)
    print(f"{name} {loss}: point ratio min {t['point_ratio'].min():.3g}, camera + z ratio {t['camera_ratio']:.3g}")
    assert not t["deficient"]
    assert t["camera_ratio"] > 1e-7  # three orders above the threshold


def test_rank_test_flags_gauge_free(pkg, orc):
    """Only arc 0 constant: the scale is free, with or without free intrinsics."""
    for name, prob in (("rig3x5-gauge", cr.rig3x5(pkg, ())), ("shape_a", ir.shape_a(pkg, orc))):
        L, A, _ = lr.jacobian(pkg, orc, prob, groups=7)
        t = czr.rank_test(A, L)
        print(f"{name}: camera + z ratio {t['camera_ratio']:.3g}")
        assert len(t["deficient_points"]) == 0
        assert t["deficient"] and abs(t["camera_ratio"]) < 1e-10


def test_constant_intrinsics_understate_the_variances(jac):
    """Why the call exists: on rig6x20 the extrinsic variances with the intrinsics held constant
    are never larger, and some are smaller by more than an order of magnitude."""
    prob, _, L, A, _ = jac("rig6x20")
    n3, n_pc = 3 * L.np, L.n_pc
    full = np.diag(cr.sigma_inv(A))[n3:n_pc]
    const = np.diag(cr.sigma_inv(A[:, :n_pc]))[n3:]
    ratio = full / const
    print(f"extrinsic variance ratios: {ratio.min():.3g} .. {ratio.max():.3g}")
    assert ratio.min() >= 1.0 and ratio.max() >= 10.0


# ---- the C ABI without a device ---------------------------------------------------------------
def test_null_handle_is_invalid(pkg):
    lib = pkg.load_library()
    info, zinfo = pkg.DabCovarianceInfo(), pkg.DabCovarianceIntrInfo()
    rc = lib.dab_covariance_intrinsics(None, None, None, None, None, None, C.byref(info), C.byref(zinfo))
    assert rc == pkg.DAB_E_INVALID
    assert "null handle" in pkg.last_error()


def test_intr_info_layout(pkg):
    assert C.sizeof(pkg.DabCovarianceIntrInfo) == 24
    assert [f for f, _ in pkg.DabCovarianceIntrInfo._fields_] == ["num_free_intr", "num_free_scalars", "border_ms",
                                                                  "reserved"]
