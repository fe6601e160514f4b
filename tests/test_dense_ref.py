"""CPU tests of the dense-Cholesky reference (tests/dense_ref.py): LAPACK on every family and
size the GPU tests (test_gpu_dense.py) use, so that the families and the metrics cannot
drift. The GPU pass rule is relative to LAPACK's own error on the same system; these pin
that error: eta_ref <= 128 eps everywhere, phi_ref <= 64 eps on blockdiag, eta_ref <= eps on
lowrank (the bound K eps of the one case too large for a LAPACK reference rests on it), and
nonpd() fails LAPACK at every index used."""
import numpy as np
import pytest

import dense_ref as dr

EPS = dr.EPS


def test_longdouble_is_extended():
    """The metrics are meant to be exact to well below eps: that needs a 64-bit mantissa."""
    assert np.finfo(dr.LD).eps <= 2.0 ** -63


@pytest.mark.parametrize("name,n,seed", dr.pinned_systems())
def test_lapack_on_family(name, n, seed):
    ref = dr.reference(name, n, seed)
    A = ref["A"]
    assert A.shape == (n, n) and np.array_equal(A, A.T) and np.all(np.isfinite(A))
    assert ref["eta_ref"] <= 128 * EPS, ref["eta_ref"] / EPS
    if name == "lowrank":
        assert ref["eta_ref"] <= EPS, ref["eta_ref"] / EPS
    if name == "blockdiag":
        assert ref["phi_ref"] <= 64 * EPS, ref["phi_ref"] / EPS


def test_family_properties():
    """What the families claim: the condition numbers, the exact zeros, the grading."""
    n = 130
    A = dr.reference("wishart", n)["A"]
    assert np.linalg.cond(A) < 10
    A = dr.reference("graded", n)["A"]
    d = np.sqrt(np.diag(A))
    assert d.max() / d.min() > 1e6 and np.linalg.cond(A / np.outer(d, d)) < 100
    A = dr.reference("spectrum", n)["A"]
    w = np.linalg.eigvalsh(A)
    assert 0.5e10 < w[-1] / w[0] < 2e10
    A = dr.reference("blockdiag", n)["A"]
    mask = np.kron(np.eye(n // dr.BLOCK + 1), np.ones((dr.BLOCK, dr.BLOCK)))[:n, :n] > 0
    assert np.all(A[~mask] == 0.0)
    scales = set()
    for o in range(0, n, dr.BLOCK):
        blk = A[o:o + dr.BLOCK, o:o + dr.BLOCK]
        assert np.linalg.cond(blk) <= 4.0 * (1 + 1e-12)
        scales.add(int(np.floor(np.log10(np.linalg.eigvalsh(blk)[0]) + 1e-9)))
    assert min(scales) <= -5 and max(scales) >= 5 and len(scales) >= 8
    A = dr.reference("lowrank", n)["A"]
    w = np.linalg.eigvalsh(A)
    assert w[0] >= 0.5 * (1 - 1e-12) and (w > 2.0 + 1e-9).sum() == 64


def test_metrics_see_a_wrong_component():
    """eta on graded sees an error of 1e-10 relative in the component of the smallest scale
    (an unscaled residual norm would not), phi_blocks sees one in the smallest block, and
    both are ~eps for LAPACK's own x."""
    ref = dr.reference("graded", 130)
    A, b = ref["A"], ref["b"]
    i = int(np.argmin(np.diag(A)))
    x = ref["x_ref"].copy()
    x[i] *= 1 + 1e-10
    assert dr.eta(A, x, b) > 1e3 * EPS >= 1e3 * ref["eta_ref"]
    r = A @ x - b
    assert np.abs(r).max() <= 1e-13 * (np.abs(A).sum(axis=1).max() * np.abs(x).max())  # unscaled: invisible
    ref = dr.reference("blockdiag", 130)
    A = ref["A"]
    i = int(np.argmin(np.diag(A)))
    x = ref["x_ref"].copy()
    x[i] *= 1 + 1e-10
    assert dr.phi_blocks(A, x, ref["x_true"]) > 1e4 * EPS
    assert dr.eta(A, np.full(130, np.nan), ref["b"]) == float("inf")


@pytest.mark.parametrize("n,j", dr.NONPD)
def test_nonpd_fails_lapack_at_j(n, j):
    A = dr.reference("wishart", n)["A"]
    B = dr.nonpd(A, j)
    with pytest.raises(np.linalg.LinAlgError):
        np.linalg.cholesky(B)
    if j > 0:  # the leading j x j part is untouched and still factors: the first bad pivot is j
        np.linalg.cholesky(B[:j, :j])
    assert np.count_nonzero(B != A) == 1


def test_lower_nan():
    A = dr.reference("wishart", 17)["A"]
    L = dr.lower_nan(A)
    iu = np.triu_indices(17, 1)
    assert np.isnan(L[iu]).all() and np.array_equal(np.tril(L), np.tril(A))
