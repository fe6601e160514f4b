"""TEST INFRASTRUCTURE ONLY: the prior sets and cases of the extrinsic-prior tests (a plain module).

A prior on extrinsic e is Ceres' NormalPrior(A, mu) with a NULL loss on that block: the residual
block r = A (x_e - mu), x_e = ext[e] as stored. The reference is lm_ref.lm / lm_ref.covariance with
`priors`, which puts the prior rows under the observations' (lm_ref.linearize). Here are the prior
sets and the cases the CPU and GPU tests share.
"""
import numpy as np

import intr_ref as ir
import lm_ref as lr
import ptconst_ref as pr
import robust_ref as rr

# ---- the shared prior sets ----------------------------------------------------------------------
SIG_W, SIG_T, SIG_POS = 0.02, 0.05, 0.01


def pose(prob, seed=11, groups=0):
    """A full prior on every free extrinsic, in L.ext_of's order: A = Q D (I + 0.2 G), Q from the QR
    of a normal draw, D = diag(1/0.02 x3, 1/0.05 x3), G a normal draw; mu = start + sigma o normal."""
    rng = np.random.default_rng(seed)
    L = lr.Layout(prob, None, groups)
    sig = np.array([SIG_W] * 3 + [SIG_T] * 3)
    idx, mu, A = [], [], []
    for e in L.ext_of:
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        G = rng.standard_normal((6, 6))
        A.append(Q @ np.diag(1.0 / sig) @ (np.eye(6) + 0.2 * G))
        mu.append(prob.ext[e] + sig * rng.standard_normal(6))
        idx.append(e)
    return np.array(idx, np.int32), np.array(mu).reshape(-1, 6), np.array(A).reshape(-1, 6, 6)


def pos3(prob, seed=11, which=None):
    """A position-only prior (zero rotation rows, I / 0.01 on the translation) on the first, the
    middle and the last free extrinsic (or on `which`); mu = the start translation + 0.01 o normal."""
    rng = np.random.default_rng(seed)
    L = lr.Layout(prob, None, 0)
    ext = L.ext_of if which is None else np.asarray(which)
    if which is None:
        ext = np.array([ext[0], ext[len(ext) // 2], ext[-1]])
    A1 = np.zeros((6, 6))
    A1[3:, 3:] = np.eye(3) / SIG_POS
    mu = prob.ext[ext].copy()
    mu[:, 3:] += SIG_POS * rng.standard_normal((len(ext), 3))
    return ext.astype(np.int32), mu, np.repeat(A1[None], len(ext), axis=0)


PRIORS = {"pose": pose, "pos3": pos3}


def shape_a7(pkg, orc):
    return ir.shape_a(pkg, orc)


# (name, case, prior set, constant mask, loss, free-intrinsic groups, max_num_iterations)
TRAJECTORIES = [
    ("B-pose", "B", "pose", None, None, 0, 25),
    ("B-pos3", "B", "pos3", None, None, 0, 25),
    ("B-pose-all", "B", "pose", "all", None, 0, 25),
    ("B-pose-third-cauchy", "B", "pose", "third", pr.CAUCHY2, 0, 15),
    ("R-pose", "R", "pose", None, None, 0, 25),
    ("R-pos3", "R", "pos3", None, None, 0, 25),
    ("R-pose-all", "R", "pose", "all", None, 0, 25),
    ("R2-pose-all", "R2", "pose", "all", None, 0, 25),
    ("Bragged-pose", "Bragged", "pose", None, None, 0, 25),
    ("A-pose-groups7", "A", "pose", None, None, 7, 25),
]
REJECTED = ("B-pose", "B-pos3", "R2-pose-all")  # trajectories with rejected steps


def traj_id(t):
    return t[0]


def make_case(pkg, orc, t):
    """(problem, priors, constant mask or None, loss, groups, iterations) of a trajectory."""
    _, case, pset, mask, loss, groups, iters = t
    prob = shape_a7(pkg, orc) if case == "A" else pr.CASES[case](pkg)
    m = pr.MASKS[mask](prob) if mask else None
    return prob, PRIORS[pset](prob), m, loss or (rr.TRIVIAL, 1.0), groups, iters
