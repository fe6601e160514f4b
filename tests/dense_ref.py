"""Matrix families, error metrics and the LAPACK reference for the direct tests of the dense
Cholesky (csrc/dab_chol.hip through dab_dense_spd_solve). Pure numpy/scipy, no GPU.
tests/test_dense_ref.py pins the families under LAPACK; tests/test_gpu_dense.py runs the
device factor on them.

Families, family(name, n, rng) -> (A, x_true); A is symmetric (exactly), positive definite:
  wishart    M M^T + n I, M n x n: condition number about 5 (the family of the first dense test)
  graded     D B D, B the unit-diagonal correlation matrix of M M^T (M n x 2n), D = 10^U(-4, 4):
             cond(A) ~ 1e16, cond(B) ~ 30. The reduced camera system without Jacobi scaling.
  spectrum   Q diag(logspace(0, -10, n)) Q^T, symmetrised: cond 1e10 (a gauge-free S under a
             small LM diagonal)
  blockdiag  6 x 6 SPD blocks, cond <= 4, each scaled by 10^k, k an integer in [-6, 6]; every
             off-diagonal tile an exact zero (the rig's S)
  lowrank    M M^T + diag(U(0.5, 2)), M n x 64: cheap to build at large n
The right-hand side is b = A x_true formed in long double and rounded; x_true is standard
normal, for graded divided by D (so that every component of D x carries weight).

Metrics, evaluated in long double with D = sqrt(diag A):
  eta(A, x, b)  = |D^-1 (A x - b)|_inf / (|D^-1 A D^-1|_inf |D x|_inf + |D^-1 b|_inf), the
             scaled normwise backward error. Cholesky is invariant under a symmetric diagonal
             scaling (up to the rounding of the scaling itself), so a correct factorisation
             keeps it at a few eps on `graded` too, where the unscaled one says nothing.
  phi_blocks(A, x, x_true), blockdiag only: the relative forward error of each 6 x 6 block in
             its own inf-norm, the maximum over the blocks. A global norm would hide a tile of
             scale 1e6 leaking into a neighbour of scale 1e-6.

nonpd(A, j): A with A[j, j] lowered by 1.001 L[j, j]^2 (L numpy's Cholesky factor): the pivots
before j are untouched and pivot j becomes -1e-3 L[j, j]^2, clear of rounding, so the first
non-positive pivot is exactly j.

Pass rule of the GPU tests: ok and eta_dev <= K max(eta_ref, eps) (on blockdiag also phi_dev
<= K max(phi_ref, eps)), eta_ref LAPACK's value on the same system (lapack_solve below).

K is one constant for every family: four times the worst ratio measured on an MI355X, rounded
up to a power of two (the factor covers the seed-to-seed spread of LAPACK's own eta, 0.1 - 0.6
eps here, and the device's other summation order). It may not exceed 64: a family that needs
more is a finding about the explicit 16 x 16 inverses of the panel solves, not a tolerance.
Measured worst eta_dev / max(eta_ref, eps) over every case of test_gpu_dense.py (MEASURED):
  wishart 1.01   graded 0.99   spectrum 0.17   lowrank 0.17   (eta_dev itself <= 1.02 eps)
  blockdiag 0.49, its phi 1.80 (phi_dev <= 3.6 eps against LAPACK's 2.4)
so K = 8 (4 x 1.80 = 7.2). Every schedule gives the same figures to two digits: the explicit
inverses cost nothing measurable on these families, cond 1e10 and 16 decades of grading included.
"""
import functools

import numpy as np
from scipy.linalg import solve_triangular

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)

FAMILIES = ("wishart", "graded", "spectrum", "blockdiag", "lowrank")
BLOCK = 6  # blockdiag's block size

# the device's worst eta_dev / max(eta_ref, eps) per family (phi for blockdiag_phi), over every
# case of tests/test_gpu_dense.py, and K from them
MEASURED = {"wishart": 1.014, "graded": 0.992, "spectrum": 0.169, "blockdiag": 0.486, "blockdiag_phi": 1.804,
            "lowrank": 0.169}
K = 8
assert K <= 64 and K >= 4 * max(MEASURED.values()) > K / 2


# the cases of tests/test_gpu_dense.py; tests/test_dense_ref.py pins LAPACK on every (family, n)
SCHEDULES = ("", "DAB_CHOL_BACK_FLOW=0", "DAB_CHOL_FUSE_PANEL=0", "DAB_CHOL_PREFACTOR=0", "DAB_CHOL_V1=1",
             "DAB_CHOL_GROUP=3", "DAB_CHOL_STRIP=0", "DAB_CHOL_GRAPH_MIN=1",
             "DAB_CHOL_STRIP=0,DAB_CHOL_GRAPH_MIN=1", "DAB_CHOL_GROUP=3,DAB_CHOL_GRAPH_MIN=1")
EDGE_SIZES = (1, 15, 17, 64, 65, 130, 200, 449, 511, 780, 1023, 1100)
EDGE_FAMILIES = ("wishart", "graded")
HARD_SIZES = (130, 449, 1000, 2050)
HARD_FAMILIES = ("spectrum", "blockdiag", "lowrank")
# (DAB_CHOL_BACK_GROUPS, n, dataflow kernel?): one work-group owning up to 4 blocks and the
# fallback at 5; 8 blocks 4 + 4 (500: a short last block) and the fallback at 9; 7 blocks
# 3/2/2, 12 blocks 4/4/4 and the fallback at 13
OWNERSHIP = ((1, 64, True), (1, 100, True), (1, 256, True), (1, 300, False),
             (2, 500, True), (2, 512, True), (2, 576, False),
             (3, 448, True), (3, 768, True), (3, 800, False))
BIG_N = 8256  # 129 blocks: work-group 0 of the 128 owns two (family lowrank, no LAPACK reference)
NONPD = ((200, 0), (200, 15), (200, 16), (200, 63), (200, 64), (200, 100), (200, 199), (1100, 700), (1100, 1099))
NONFINITE_SIZES = (130, 1100)
SEQUENCE = ((2050, 0), (1000, 0), (130, 0), (2050, 1))  # (n, seed) on one handle, family wishart;
SEQUENCE_NONPD = (1100, 700)                             # then nonpd 1100, then 1100 positive definite
INTERLEAVED_N = 1020


def pinned_systems():
    """Every positive definite (family, n, seed) the GPU tests compare with LAPACK."""
    out = [(f, n, 0) for f in EDGE_FAMILIES for n in EDGE_SIZES]
    out += [(f, n, 0) for f in HARD_FAMILIES for n in HARD_SIZES]
    out += [("wishart", n, 0) for _, n, _ in OWNERSHIP]
    out += [("wishart", n, s) for n, s in SEQUENCE] + [("wishart", 1100, 0), ("wishart", INTERLEAVED_N, 0)]
    out += [("wishart", n, 0) for n in NONFINITE_SIZES]
    return sorted(set(out))


def _orth(n, rng):
    q, r = np.linalg.qr(rng.standard_normal((n, n)))
    return q * np.sign(np.diag(r))


def family(name, n, rng):
    """(A, x_true) of the named family; A float64, exactly symmetric."""
    x_true = rng.standard_normal(n)
    if name == "wishart":
        M = rng.standard_normal((n, n))
        A = M @ M.T + n * np.eye(n)
    elif name == "graded":
        M = rng.standard_normal((n, 2 * n))
        W = M @ M.T
        W = 0.5 * (W + W.T)
        d = np.sqrt(np.diag(W))
        B = W / np.outer(d, d)
        np.fill_diagonal(B, 1.0)
        D = 10.0 ** rng.uniform(-4.0, 4.0, n)
        A = B * np.outer(D, D)  # D_i D_j commutes, so A stays exactly symmetric
        x_true = x_true / D
    elif name == "spectrum":
        Q = _orth(n, rng)
        A = (Q * np.logspace(0.0, -10.0, n)) @ Q.T
    elif name == "blockdiag":
        A = np.zeros((n, n))
        for o in range(0, n, BLOCK):
            m = min(BLOCK, n - o)
            Q = _orth(m, rng)
            S = (Q * rng.uniform(1.0, 4.0, m)) @ Q.T
            A[o:o + m, o:o + m] = S * 10.0 ** int(rng.integers(-6, 7))
    elif name == "lowrank":
        M = rng.standard_normal((n, 64))
        A = M @ M.T
        A[np.diag_indices(n)] += rng.uniform(0.5, 2.0, n)
    else:
        raise ValueError(name)
    A = 0.5 * (A + A.T)
    return A, x_true


def _rows(n, step=512):
    for o in range(0, n, step):
        yield slice(o, min(n, o + step))


def rhs(A, x_true):
    """b = A x_true in long double, rounded to float64 (row chunks: A is never copied whole)."""
    x = x_true.astype(LD)
    b = np.empty(A.shape[0])
    for s in _rows(A.shape[0]):
        b[s] = (A[s].astype(LD) @ x).astype(np.float64)
    return b


def system(name, n, seed=0):
    """(A, b, x_true) of family `name` at size n; the seed fixes the draw."""
    rng = np.random.default_rng([seed, n, FAMILIES.index(name)])
    A, x_true = family(name, n, rng)
    return A, rhs(A, x_true), x_true


def eta(A, x, b):
    """The scaled normwise backward error of x for A x = b (module docstring), a float.
    A non-finite x gives inf."""
    if not np.all(np.isfinite(x)):
        return float("inf")
    n = A.shape[0]
    D = np.sqrt(np.diag(A).astype(LD))
    s = 1.0 / D
    xl, bl = x.astype(LD), b.astype(LD)
    num, nrm = LD(0), LD(0)
    for r in _rows(n):
        Al = A[r].astype(LD)
        num = max(num, np.abs(s[r] * (Al @ xl - bl[r])).max())
        nrm = max(nrm, ((np.abs(Al) @ s) * s[r]).max())
    den = nrm * np.abs(D * xl).max() + np.abs(s * bl).max()
    return float(num / den)


def phi_blocks(A, x, x_true):
    """blockdiag: max over the 6 x 6 blocks of |x - x_true|_inf / |x_true|_inf within the block."""
    if not np.all(np.isfinite(x)):
        return float("inf")
    n = A.shape[0]
    worst = LD(0)
    xl, tl = x.astype(LD), x_true.astype(LD)
    for o in range(0, n, BLOCK):
        s = slice(o, min(n, o + BLOCK))
        worst = max(worst, np.abs(xl[s] - tl[s]).max() / np.abs(tl[s]).max())
    return float(worst)


def lapack_solve(A, b):
    """x from LAPACK's Cholesky (dpotrf) and two triangular solves (dtrtrs); raises
    numpy.linalg.LinAlgError when A is not positive definite."""
    L = np.linalg.cholesky(A)
    z = solve_triangular(L, b, lower=True, check_finite=False)
    return solve_triangular(L, z, lower=True, trans="T", check_finite=False)


@functools.lru_cache(maxsize=None)
def reference(name, n, seed=0):
    """The system and LAPACK's result on it, computed once and shared (read-only arrays):
    dict A, b, x_true, x_ref, eta_ref, phi_ref (blockdiag; else None)."""
    A, b, x_true = system(name, n, seed)
    x_ref = lapack_solve(A, b)
    for a in (A, b, x_true, x_ref):
        a.setflags(write=False)
    return {"A": A, "b": b, "x_true": x_true, "x_ref": x_ref, "eta_ref": eta(A, x_ref, b),
            "phi_ref": phi_blocks(A, x_ref, x_true) if name == "blockdiag" else None}


def nonpd(A, j):
    """A with pivot j of its Cholesky factorisation turned to -1e-3 of its value."""
    L = np.linalg.cholesky(A)
    B = A.copy()
    B[j, j] -= 1.001 * L[j, j] ** 2
    return B


def lower_nan(A):
    """What the device gets: A's lower triangle, the strict upper triangle NaN (the library
    documents that it reads the lower triangle only; a NaN shows any read of the rest)."""
    out = np.array(A)
    for i in range(A.shape[0] - 1):
        out[i, i + 1:] = np.nan
    return out
