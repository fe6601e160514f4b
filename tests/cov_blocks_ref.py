"""TEST INFRASTRUCTURE ONLY: the reference of dab_covariance_blocks (a plain module).

The cross blocks of Sigma = (J^T J)^-1 between a point and another point, an extrinsic or an
intrinsic are slices of the full Sigma that cov_ref.sigma_inv gives for the dense Jacobian of
lm_ref.jacobian over lm_ref.Layout (ptprior_ref.jacobian where point priors are set,
extsub_ref.jacobian over extsub_ref.SubLayout where a scalar mask is set, with exact-zero rows and
columns put back), cut by the layout's columns:
  pp (a, b)  Sigma[3 i_a : +3, 3 i_b : +3], i = the place of the point in Layout.pt_of
  pe (p, e)  Sigma[3 i_p : +3, 3 np + 6 c : +6], c = the place of e in Layout.ext_of
  pz (p, z)  3x6 over the slots (cx, cy, f0, f1, k0, k1): the columns of z's active scalars, 0 elsewhere
Known exactly (0, and `exact` marks the entries): a referenced constant point, a constant
extrinsic (ext_const, freeze_camera), a constant scalar of an extrinsic, an inactive slot, an
intrinsic without a free scalar. No information (NaN): a point no observation references, a
non-constant extrinsic nothing references. NaN goes before 0.

schur_blocks is the second, independent statement of the same blocks: the three Schur formulas of
the library's route in numpy from the Cholesky factors of the point blocks, the
records Y and C = S^-1 in the Jacobi-scaled variables. tests/test_cov_blocks_ref.py pins the
slices against cov_ref.sigma_pinv, schur_blocks against the slices, and shows that compare()
fails on the mistakes a kernel can make (`wrong` of schur_blocks).
"""
import numpy as np

import cov_ref as cr
import extsub_ref as xr
import lm_ref as lr
import ptprior_ref as ppr

BOUND_FACTOR = 64.0


def reference(pkg, orc, prob, *, bits=None, priors=None, point_priors=None, const=None, groups=0,
              loss=lr.TRIVIAL):
    """Everything a test compares against, computed once per case: the layout, the dense Jacobian
    over its (free) columns, Sigma over the full layout (constant scalars: zero rows and columns),
    kappa of the scaled H, m = max |Sigma| and the bound 64 kappa 2^-53 m."""
    if bits is not None:
        assert point_priors is None
        L, A, cost = xr.jacobian(pkg, orc, prob, bits=bits, priors=priors, const=const, groups=groups, loss=loss)
    else:
        L, A, cost = ppr.jacobian(pkg, orc, prob, priors=priors, point_priors=point_priors, const=const,
                                  groups=groups, loss=loss)
    Sigma = cr.sigma_inv(A)
    if hasattr(L, "expand"):
        Sigma = L.expand(Sigma)
    kappa = cr.kappa(A)
    m = float(np.abs(Sigma).max())
    return dict(layout=L, A=A, Sigma=Sigma, kappa=kappa, m=m, bound=BOUND_FACTOR * kappa * cr.EPS * m, cost=cost,
                prob=prob)


class Index:
    """Where the caller's ids sit in the full layout (3 np point columns, 6 nc camera columns, nz
    intrinsic scalars): -1 = known exactly, -2 = no information."""

    def __init__(self, L, prob):
        npts, next_, ni = prob.points.shape[0], prob.ext.shape[0], prob.intr.shape[0]
        self.n3 = 3 * L.np
        self.ncam = 6 * L.nc
        self.pt = np.full(npts, -2, np.int64)
        self.pt[L.const_of] = -1
        self.pt[L.pt_of] = np.arange(L.np)
        econst = np.zeros(next_, bool) if prob.ext_const is None else prob.ext_const.astype(bool)
        if prob.freeze_camera:
            econst[:] = True
        self.ext = np.full(next_, -2, np.int64)
        self.ext[econst] = -1
        self.ext[L.ext_of] = np.arange(L.nc)
        # column of slot k of intrinsic i, -1 where the slot is not an unknown
        self.zcol = -np.ones((ni, 6), np.int64)
        self.zcol[L.zi, L.zk] = self.n3 + self.ncam + np.arange(L.nz)
        # constant scalars of the free extrinsics (SubLayout): [nc][6] free
        self.ext_free = getattr(L, "ext_free", np.ones((L.nc, 6), bool))


def slices(ref, pp=(), pe=(), pz=()):
    """(blocks, exact): dicts of pp [n][3][3], pe [n][3][6], pz [n][3][6] cut from ref["Sigma"],
    and bool arrays of the same shapes marking the entries that are known exactly (0)."""
    L, S = ref["layout"], ref["Sigma"]
    ix = Index(L, ref["prob"])
    pp, pe, pz = (np.asarray(x, np.int64).reshape(-1, 2) for x in (pp, pe, pz))
    out = dict(pp=np.zeros((len(pp), 3, 3)), pe=np.zeros((len(pe), 3, 6)), pz=np.zeros((len(pz), 3, 6)))
    exact = {k: np.zeros(v.shape, bool) for k, v in out.items()}
    for i, (a, b) in enumerate(pp):
        ia, ib = ix.pt[a], ix.pt[b]
        if ia == -2 or ib == -2:
            out["pp"][i] = np.nan
        elif ia == -1 or ib == -1:
            exact["pp"][i] = True
        else:
            out["pp"][i] = S[3 * ia:3 * ia + 3, 3 * ib:3 * ib + 3]
    for i, (a, e) in enumerate(pe):
        ia, c = ix.pt[a], ix.ext[e]
        if ia == -2 or c == -2:
            out["pe"][i] = np.nan
        elif ia == -1 or c == -1:
            exact["pe"][i] = True
        else:
            o = ix.n3 + 6 * c
            out["pe"][i] = S[3 * ia:3 * ia + 3, o:o + 6]
            exact["pe"][i][:, ~ix.ext_free[c]] = True
    for i, (a, z) in enumerate(pz):
        ia = ix.pt[a]
        if ia == -2:
            out["pz"][i] = np.nan
        elif ia == -1:
            exact["pz"][i] = True
        else:
            for k in range(6):
                c = ix.zcol[z, k]
                if c >= 0:
                    out["pz"][i][:, k] = S[3 * ia:3 * ia + 3, c]
                else:
                    exact["pz"][i][:, k] = True
    for k in out:
        assert (out[k][exact[k]] == 0.0).all()
    return out, exact


# ---- the route's algebra, stated independently of the slices ---------------------------------------
def schur_parts(ref):
    """The ingredients of the library's route from the dense Jacobian, in the Jacobi-scaled
    variables over the full layout: s (0 for a constant scalar), per free point PU_p = s_p L_p^-T
    and its records [(columns of the camera part, Y 6x3 or narrower)], one per camera or free
    intrinsic with a non-zero block, and C = S^-1 over the camera part (a unit diagonal where a
    scalar is constant)."""
    L, A = ref["layout"], ref["A"]
    n_full = getattr(L, "n_full", L.n)
    keep = getattr(L, "keep", np.arange(L.n))
    Af = np.zeros((A.shape[0], n_full))
    Af[:, keep] = A
    s = np.zeros(n_full)
    s[keep] = cr.jacobi_scale(A)
    As = Af * s
    H = As.T @ As
    n3, ncam = 3 * L.np, 6 * L.nc
    held = np.ones(n_full, bool)
    held[keep] = False
    S = H[n3:, n3:] + np.diag(held[n3:].astype(float))
    groups = [np.arange(6 * c, 6 * c + 6) for c in range(L.nc)]
    for i in np.unique(L.zi):
        groups.append(ncam + np.flatnonzero(L.zi == i))
    PU, recs = [], []
    for p in range(L.np):
        k = slice(3 * p, 3 * p + 3)
        Lp = np.linalg.cholesky(H[k, k])
        LiT = np.linalg.inv(Lp).T
        PU.append(np.diag(s[k]) @ LiT)
        Y = H[n3:, k] @ LiT
        S -= Y @ Y.T
        recs.append([(g, Y[g]) for g in groups if Y[g].any()])
    return dict(s=s, PU=PU, recs=recs, C=np.linalg.inv(S), groups=groups, n3=n3, ncam=ncam)


def schur_blocks(ref, parts, pp=(), pe=(), pz=(), wrong=None):
    """The three formulas for the same pairs as slices(), free points and free columns
    only (the rest is slices()'s bookkeeping and is copied from it):
      Sigma_pp' = PU_p (delta I + sum_r sum_r' Y_r^T C_rr' Y_r') PU_p'^T
      Sigma_pc  = -PU_p (sum_r Y_r^T C_r,c) diag(s_c)
    wrong: one of the mistakes compare() must catch: "transpose" (a pp block transposed),
    "sign" (pe / pz without the minus), "scale" (without s), "record" (the first record of the
    point dropped), "order" ((a, b) answered with PU and records of (b, a))."""
    L = ref["layout"]
    ix = Index(L, ref["prob"])
    out, exact = slices(ref, pp, pe, pz)
    out = {k: v.copy() for k, v in out.items()}
    pp, pe, pz = (np.asarray(x, np.int64).reshape(-1, 2) for x in (pp, pe, pz))
    C, s, PU = parts["C"], parts["s"], parts["PU"]

    def recs(p):
        r = parts["recs"][p]
        return r[1:] if wrong == "record" else r

    def pc(ia, cols):
        acc = np.zeros((3, len(cols)))
        for g, Y in recs(ia):
            acc += Y.T @ C[np.ix_(g, cols)]
        sc = np.ones(len(cols)) if wrong == "scale" else s[parts["n3"] + cols]
        return (1.0 if wrong == "sign" else -1.0) * PU[ia] @ acc * sc

    for i, (a, b) in enumerate(pp):
        ia, ib = ix.pt[a], ix.pt[b]
        if ia < 0 or ib < 0:
            continue
        if wrong == "order":
            ia, ib = ib, ia
        M = np.eye(3) * float(ia == ib)
        for g, Y in recs(ia):
            for h, Z in recs(ib):
                M += Y.T @ C[np.ix_(g, h)] @ Z
        blk = PU[ia] @ M @ PU[ib].T
        out["pp"][i] = blk.T if wrong == "transpose" else blk
    for i, (a, e) in enumerate(pe):
        ia, c = ix.pt[a], ix.ext[e]
        if ia < 0 or c < 0:
            continue
        blk = pc(ia, np.arange(6 * c, 6 * c + 6))
        if wrong != "scale":
            blk[:, ~ix.ext_free[c]] = 0.0
        out["pe"][i] = blk
    for i, (a, z) in enumerate(pz):
        ia = ix.pt[a]
        slots = np.flatnonzero(ix.zcol[z] >= 0)
        if ia < 0 or len(slots) == 0:
            continue
        out["pz"][i][:, slots] = pc(ia, ix.zcol[z, slots] - parts["n3"])
    return out, exact


# ---- the comparator ----------------------------------------------------------------------------------
def compare(got, want, exact, bound):
    """Largest |got - want| over the three kinds as a fraction of the bound. AssertionError when a
    shape differs, a NaN is misplaced, an entry known exactly is not +0, or the bound is missed."""
    worst = 0.0
    for k in ("pp", "pe", "pz"):
        g, w = np.asarray(got[k]), want[k]
        assert g.shape == w.shape, (k, g.shape, w.shape)
        if not w.size:
            continue
        nan = np.isnan(w)
        assert (np.isnan(g) == nan).all(), f"{k}: NaN pattern"
        ex = exact[k]
        assert (g[ex] == 0.0).all() and not np.signbit(g[ex]).any(), f"{k}: an entry known exactly is not +0"
        err = float(np.abs(np.where(nan, 0.0, g - w)).max())
        assert err <= bound, f"{k}: error {err:.3e} above the bound {bound:.3e}"
        worst = max(worst, err / bound)
    return worst


# ---- pair lists ----------------------------------------------------------------------------------------
def pair_lists(prob, seed, npp=24, npe=36, npz=24):
    """Seeded lists over all point, extrinsic and intrinsic ids (constant and unreferenced ones
    included): pp with (a, a), (a, b) beside (b, a) and a duplicate; pe with every extrinsic of
    three observations (pairs the point sees) beside random ones; pz over all intrinsics, with the
    intrinsic of three observations."""
    rng = np.random.default_rng(seed)
    npts, next_, ni = prob.points.shape[0], prob.ext.shape[0], prob.intr.shape[0]
    ab = rng.integers(0, npts, (npp, 2))
    pp = np.concatenate([ab, ab[:4, ::-1], ab[:2], np.stack([ab[:4, 0], ab[:4, 0]], axis=1), [[0, 0], [0, 1]]])
    obs = rng.integers(0, prob.num_obs, 3)
    seen = [(prob.obs_point[o], prob.obs_ext0[o]) for o in obs]
    seen += [(prob.obs_point[o], prob.obs_ext1[o]) for o in obs if prob.obs_ext1[o] >= 0]
    pe = np.concatenate([np.array(seen, np.int64).reshape(-1, 2),
                         np.stack([rng.integers(0, npts, npe), rng.integers(0, next_, npe)], axis=1),
                         [[0, 0], [1, next_ - 1]]])
    pz = np.concatenate([np.array([(prob.obs_point[o], prob.obs_intr[o]) for o in obs], np.int64).reshape(-1, 2),
                         np.stack([rng.integers(0, npts, npz), rng.integers(0, ni, npz)], axis=1), [[0, 0]]])
    return pp.astype(np.int32), pe.astype(np.int32), pz.astype(np.int32)
