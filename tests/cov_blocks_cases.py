"""TEST INFRASTRUCTURE ONLY: the cases the CPU and GPU tests of dab_covariance_blocks share (a
plain module). Each is the smallest cov_ref / cov_intr_ref / ptconst_ref / extsub_ref / ptprior_ref
problem that reaches one path of the call:
  rig3x5               n = 30, tiles, arc∘ring observations (two entries per observation, repeated
                       cameras in a point's records)
  bal40 | bal170       tiles | pair tables
  bal40-ragged         points with 2 to 8 records, an unreferenced point
  freeze               no camera: Sigma_pp' = delta V^-1, every pe block +0
  rig6x20-mixed-g7     every group free on every intrinsic: pz pairs for an intrinsic the point sees
                       and for one it does not, inactive slots
  rig6x20-mixed-masks  masks [7, 0, 2, 5, 0, 4]: intrinsics outside the free set
  bal40-first16        16 of 40 intrinsics free, the border sums in global memory
  cauchy               rig6x20-mixed-g7 under Cauchy(2.0)
  ptconst-third        ptconst_ref's B with every third point constant
  extsub-trans-all     extsub_ref's Blow with every translation constant
  soft-gauge           cov_ref.bal40(()), gauge-free, with prior_ref.pos3 and ptprior_ref.gcp3
"""
import numpy as np

import cov_blocks_ref as cbr
import cov_intr_ref as czr
import cov_ref as cr
import extsub_ref as xr
import lm_ref as lr
import prior_ref as qr
import ptconst_ref as pr
import ptprior_ref as ppr
import robust_ref as rr


def _plain(make):
    return lambda pkg: dict(prob=make(pkg))


def _intr(name, **kw):
    def make(pkg):
        prob, groups = czr.CASES[name](pkg)
        return dict(prob=prob, groups=groups, **kw)
    return make


def _ptconst(pkg):
    prob = pr.case_b(pkg)
    return dict(prob=prob, const=pr.every_third(prob))


def _extsub(pkg):
    prob = xr.CASES["Blow"](pkg)
    return dict(prob=prob, bits=xr.trans_all(prob))


def _soft_gauge(pkg):
    prob = cr.bal40(pkg, ())
    return dict(prob=prob, priors=qr.pos3(prob), point_priors=ppr.gcp3(prob, ppr.truth(pkg, "bal40")))


CASES = {
    "rig3x5": _plain(cr.rig3x5), "bal40": _plain(cr.bal40), "bal170": _plain(cr.bal170),
    "bal40-ragged": _plain(cr.bal40_ragged), "freeze": _plain(cr.freeze),
    "rig6x20-mixed-g7": _intr("rig6x20-mixed"), "rig6x20-mixed-masks": _intr("rig6x20-mixed-masks"),
    "bal40-first16": _intr("bal40-first16", env={"DAB_INTR_BORDER_LDS": "0"}),
    "cauchy": _intr("rig6x20-mixed", loss=(rr.CAUCHY, 2.0)),
    "ptconst-third": _ptconst, "extsub-trans-all": _extsub, "soft-gauge": _soft_gauge,
}
LOSS_NAMES = {rr.HUBER: "huber", rr.CAUCHY: "cauchy"}


def spec(pkg, name):
    d = dict(groups=0, loss=None, const=None, bits=None, priors=None, point_priors=None, env={})
    d.update(CASES[name](pkg))
    return d


def reference(pkg, orc, name):
    """cov_blocks_ref.reference of a case, with its spec under "spec"."""
    sp = spec(pkg, name)
    ref = cbr.reference(pkg, orc, sp["prob"], bits=sp["bits"], priors=sp["priors"], point_priors=sp["point_priors"],
                        const=sp["const"], groups=sp["groups"], loss=sp["loss"] or lr.TRIVIAL)
    ref["spec"] = sp
    return ref


def solver(pkg, sp, **kw):
    """A Solver with the case's problem (a copy), loss, masks, priors and free set on it."""
    s = pkg.Solver(0, **kw)
    try:
        if sp["loss"]:
            s.set_loss(LOSS_NAMES[sp["loss"][0]], sp["loss"][1])
        s.set_problem(sp["prob"].copy())
        if np.any(sp["groups"]):
            s.set_intrinsics_free(sp["groups"])
        if sp["const"] is not None:
            s.set_points_constant(sp["const"])
        if sp["bits"] is not None:
            s.set_ext_scalars_constant(sp["bits"])
        if sp["priors"] is not None:
            s.set_ext_priors(*sp["priors"])
        if sp["point_priors"] is not None:
            s.set_point_priors(*sp["point_priors"])
    except Exception:
        s.close()
        raise
    return s
