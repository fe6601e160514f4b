"""What constant scalars of the extrinsics cost at run time: the LM iteration without a mask and with
every translation constant (DAB_EXT_TRANSLATION on every extrinsic, tests/extsub_ref.py's
`trans-all`), on one handle (the sibling of scripts/prior_cost.py).

  C3 (BAL, 1000 cameras): the EXPLICIT and the PCG LM iteration;
  C5 (rig 16 x 64, 10M observations): the EXPLICIT LM iteration.
Convention (prior_cost.py's): a warmed handle, then --reps solves of up to --lm-iters LM iterations
from the same start with all tolerances 0, the variants in turn; per solve the median host
wall-clock per LM iteration. Prints one JSON line. The expectation from the code: the masked forms
replace three small launches one for one (k_scale_cams once per solve, k_cam_candidate and two
k_cam_norms per iteration) and one k_ext_unit_diag launch over 6 NC lanes is added per iteration, so
parity within the machine's noise. The two variants walk different trajectories (other unknowns), so
their counts of rejected steps, which skip the Jacobian pass, are printed beside the times.
--variants none measures the unmasked path alone and calls nothing this feature added: the same
file runs on a tree without it, for the comparison of the unchanged paths.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_iteration_ms(summary):
    t = [it["time"] for it in summary["iterations"][1:]]
    return 1e3 * float(np.median(t)) if t else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lm-iters", type=int, default=10)
    ap.add_argument("--legs", default="c3_1kcam:explicit,c3_1kcam:pcg,c5_rig_16x64:explicit")
    ap.add_argument("--variants", default="none,trans-all")
    a = ap.parse_args()
    import torch  # noqa: F401  (the GPU runtime is initialised before libdab loads)
    torch.cuda.is_available()
    import _pkgload
    pkg = _pkgload.load()
    tol0 = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    variants = tuple(a.variants.split(","))
    out = {}
    for leg in a.legs.split(","):
        config, solver = leg.split(":")
        lst = {"explicit": pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, "pcg": pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG}[solver]
        prob = pkg.synth(**pkg.CONFIGS[config])
        start = prob.copy()
        opts = pkg.options(max_num_iterations=a.lm_iters, linear_solver_type=lst, **tol0)
        s = pkg.Solver(0)
        s.set_problem(prob)
        rec = {v: [] for v in variants}
        info = {}
        for rep in range(a.reps + 1):  # interleaved; the first round warms up
            for which in variants:
                if which != "none":
                    s.set_ext_scalars_constant(0x38)
                elif len(variants) > 1:
                    s.set_ext_scalars_constant(None)
                s.update_parameters(start.points, start.ext)
                r = s.solve(opts)
                if rep:
                    rec[which].append(round(median_iteration_ms(r), 4))
                    info[which] = dict(iterations=r["num_iterations"], rejected=r["num_unsuccessful_steps"],
                                       num_parameters=r["num_parameters"], initial_cost=r["initial_cost"],
                                       final_cost=r["final_cost"], termination=r["termination"],
                                       schur_assembly=r["schur_assembly"])
        s.close()
        med = {k: float(np.median(v)) for k, v in rec.items() if v}
        out[leg] = dict(lm_iteration_ms=rec, lm_iteration_ms_median=med,
                        ratio_to_none={k: round(v / med["none"], 4) for k, v in med.items()} if "none" in med else {},
                        **info)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
