"""TEST INFRASTRUCTURE ONLY: records tests/golden/lm_ref_parent.json, the pin of tests/lm_ref.py.

tests/lm_ref.lm replaced four copies of the reference trust-region loop (robust_ref.lm, intr_ref.lm,
ptconst_ref.lm, prior_ref.lm). The file holds what those four functions returned at commit PARENT, the
last one that had them, on the cases below; it was recorded there with a throwaway lm_ref.lm that
forwarded to the copy a case is listed under. Run on a tree that has tests/lm_ref.py, this script
calls lm_ref.lm only, and on the recording machine it reproduces the file byte for byte.
tests/test_lm_ref.py compares lm_ref.lm against the file by the oracle-pin rule (not bitwise:
another machine's BLAS sums in another order).

Per case: the summary without `iterations`; per iteration success, valid (0 / 1) and cost,
cost_change, gradient_max_norm, step_norm, relative_decrease, trust_region_radius as float.hex();
the final ext, intr and the first 16 referenced points as the hex digits of their float64 bit
patterns, 16 per value (float.hex() of them would put the file over its size limit).

Usage: python oracle/gen_lm_ref_golden.py [output file]
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _pkgload  # noqa: E402
import oracle  # noqa: E402

import intr_ref as ir  # noqa: E402
import lm_ref  # noqa: E402
import prior_ref as qr  # noqa: E402
import ptconst_ref as pr  # noqa: E402
import robust_ref as rr  # noqa: E402

PARENT = "e8a63275bbe7aacbe0e09cbd54fa03e65f305e05"
OUT = os.path.join(ROOT, "tests", "golden", "lm_ref_parent.json")
FLAGS = ("success", "valid")
FLOATS = ("cost", "cost_change", "gradient_max_norm", "step_norm", "relative_decrease", "trust_region_radius")
NUM_POINTS = 16


def _opts(pkg, iters, **kw):
    return pkg.options(max_num_iterations=iters, num_threads=4,
                       linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, **kw)


def cases(pkg, orc):
    """[(name, make)]: make() -> (problem, options, keyword arguments of lm_ref.lm). The name's
    first part is the copy of the loop the case was recorded from."""
    out = []
    trivial = (rr.TRIVIAL, 1.0)
    # robust_ref.lm and intr_ref.lm, with the options of their CPU tests (function_tolerance 1e-12:
    # the small problems would stop before any step is rejected otherwise)
    for pname, make in (("bal_small", rr.bal_small), ("rig_small", rr.rig_small)):
        for lname, loss in (("trivial", trivial), ("huber1", (rr.HUBER, 1.0)), ("cauchy0.5", (rr.CAUCHY, 0.5))):
            out.append((f"robust/{pname}-{lname}", lambda make=make, loss=loss: (
                make(pkg, orc)[0], _opts(pkg, 15, function_tolerance=1e-12), dict(loss=loss))))
    for sname, make, groups, loss in (("shape_a-7", ir.shape_a, 7, trivial), ("shape_b-5", ir.shape_b, 5, trivial),
                                      ("shape_c-2", ir.shape_c, 2, trivial)):
        out.append((f"intr/{sname}", lambda make=make, groups=groups, loss=loss: (
            make(pkg, orc), _opts(pkg, 15, function_tolerance=1e-12), dict(groups=groups, loss=loss))))
    out.append(("intr/shape_a-7-contaminated-cauchy0.5", lambda: (
        ir.shape_a(pkg, orc, contaminated=True), _opts(pkg, 15, function_tolerance=1e-12),
        dict(groups=7, loss=(rr.CAUCHY, 0.5)))))

    # ptconst_ref.lm
    def masked(t):
        case, mask, loss, iters = t
        prob = pr.CASES[case](pkg)
        return prob, _opts(pkg, iters), dict(const=pr.MASKS[mask](prob), loss=loss or trivial)
    for t in pr.TRAJECTORIES + [pr.RAGGED]:
        out.append((f"ptconst/{pr.traj_id(t)}", lambda t=t: masked(t)))

    def under_a_mask():  # test_free_intrinsics_layout
        prob = ir.shape_a(pkg, orc)
        return prob, _opts(pkg, 6), dict(const=pr.every_third(prob), groups=7)

    def no_free_parameter():  # test_no_free_parameter
        prob = pr.case_b(pkg)
        prob.freeze_camera = True
        return prob, _opts(pkg, 25), dict(const=True)
    out.append(("ptconst/shape_a-third-groups7", under_a_mask))
    out.append(("ptconst/B-freeze-all", no_free_parameter))

    # prior_ref.lm
    def with_priors(t):
        prob, priors, m, loss, groups, iters = qr.make_case(pkg, orc, t)
        return prob, _opts(pkg, iters), dict(priors=priors, const=m, groups=groups, loss=loss)
    for t in qr.TRAJECTORIES:
        out.append((f"prior/{qr.traj_id(t)}", lambda t=t: with_priors(t)))
    return out


def _hex(a):
    """The array's float64 values as one string, 16 hex digits each (IEEE-754 bits, most significant first)."""
    return np.ascontiguousarray(a, ">f8").tobytes().hex()


def unhex(s):
    return np.frombuffer(bytes.fromhex(s), ">f8").astype(np.float64)


def first_points(prob):
    """Indices of the first NUM_POINTS referenced points."""
    return np.unique(prob.obs_point)[:NUM_POINTS]


def record(summary, prob):
    rec = {k: (float(v).hex() if isinstance(v, (float, np.floating)) else v)
           for k, v in summary.items() if k != "iterations"}
    rec["iterations"] = [[int(it[k]) for k in FLAGS] + [float(it[k]).hex() for k in FLOATS]
                         for it in summary["iterations"]]
    rec.update(ext=_hex(prob.ext), intr=_hex(prob.intr), points=_hex(prob.points[first_points(prob)]))
    return rec


def main(path):
    pkg = _pkgload.load()
    header = dict(recorded_from=PARENT,
                  functions="robust_ref.lm, intr_ref.lm, ptconst_ref.lm, prior_ref.lm (the case name's first part)",
                  iteration_fields=list(FLAGS + FLOATS), points=f"the first {NUM_POINTS} referenced points",
                  floats="float.hex() in the summary and the iterations; ext, intr, points: 16 hex digits of the float64 "
                         "bit pattern per value, row-major", generator="oracle/gen_lm_ref_golden.py")
    lines = []
    for name, make in cases(pkg, oracle):
        prob, opts, kw = make()
        s = lm_ref.lm(pkg, oracle, prob, opts, **kw)
        lines.append(json.dumps(name) + ": " + json.dumps(record(s, prob), separators=(",", ":")))
        print(name, s["termination"], s["num_iterations"], s["num_unsuccessful_steps"], flush=True)
    with open(path, "w") as f:
        f.write('{\n"header": ' + json.dumps(header) + ',\n"cases": {\n' + ",\n".join(lines) + "\n}\n}\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else OUT)
