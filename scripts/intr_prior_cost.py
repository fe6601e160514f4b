"""What intrinsic priors cost at run time: free intrinsics without priors and with a calibration prior
on every intrinsic, on one handle (the sibling of scripts/prior_cost.py and pt_prior_cost.py).

  C5 (rig 16 x 64, 10M observations, 16 intrinsics, all groups free): the EXPLICIT LM iteration,
  the only step free intrinsics take.
Convention (prior_cost.py's): a warmed handle, then --reps solves of up to --lm-iters LM iterations
from the same start with all tolerances 0, the two variants in turn; per solve the median host
wall-clock per LM iteration. Prints one JSON line. The expectation from the code: two launches of
one work-group each per accepted iteration (k_zprior_blocks after the intrinsic sums,
k_zprior_candidate after the candidate pass) over at most 16 records of 63 doubles, so a few
microseconds of launch latency against an iteration of several milliseconds.
--trace-only runs one solve with the priors and nothing else (for a kernel trace).
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


def calib_priors(prob, seed=11):
    """tests/intrprior_ref.py's `calib` on every intrinsic: A = Q diag(1 / sigma) (I + 0.2 G), sigma =
    (2, 2, 5e-3 |f0|, 5e-3 |f1|, 5e-3, 5e-3) with a zero replaced by 1, mean = start + sigma o normal."""
    rng = np.random.default_rng(seed)
    idx, mu, A = [], [], []
    for i, k6 in enumerate(prob.intr):
        sig = np.array([2.0, 2.0, 5e-3 * abs(k6[2]), 5e-3 * abs(k6[3]), 5e-3, 5e-3])
        sig[sig == 0.0] = 1.0
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        G = rng.standard_normal((6, 6))
        A.append(Q @ np.diag(1.0 / sig) @ (np.eye(6) + 0.2 * G))
        mu.append(k6 + sig * rng.standard_normal(6))
        idx.append(i)
    return np.array(idx, np.int32), np.array(mu).reshape(-1, 6), np.array(A).reshape(-1, 6, 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lm-iters", type=int, default=10)
    ap.add_argument("--config", default="c5_rig_16x64")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (the GPU runtime is initialised before libdab loads)
    torch.cuda.is_available()
    import _pkgload
    pkg = _pkgload.load()
    tol0 = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    prob = pkg.synth(**pkg.CONFIGS[a.config])
    start = prob.copy()
    priors = calib_priors(start)
    variants = ("calib",) if a.trace_only else ("none", "calib")
    opts = pkg.options(max_num_iterations=a.lm_iters, linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, **tol0)
    s = pkg.Solver(0)
    s.set_problem(prob)
    s.set_intrinsics_free(7)
    rec = {v: [] for v in variants}
    info = {}
    for rep in range(1 if a.trace_only else a.reps + 1):  # interleaved; the first round warms up
        for which in variants:
            s.set_intr_priors(*priors) if which == "calib" else s.set_intr_priors(None)
            s.update_parameters(start.points, start.ext)
            s.update_intrinsics(start.intr)
            r = s.solve(opts)
            if rep or a.trace_only:
                rec[which].append(round(median_iteration_ms(r), 4))
                info[which] = dict(iterations=r["num_iterations"], rejected=r["num_unsuccessful_steps"],
                                   num_residuals=r["num_residuals"], num_parameters=r["num_parameters"],
                                   initial_cost=r["initial_cost"], final_cost=r["final_cost"],
                                   termination=r["termination"], schur_assembly=r["schur_assembly"])
    effective = s.get_intr_priors()[3]
    s.close()
    med = {k: float(np.median(v)) for k, v in rec.items() if v}
    out = {a.config + "_explicit_groups7": dict(
        lm_iteration_ms=rec, num_intrinsics=int(start.intr.shape[0]), effective_priors_last=int(effective),
        lm_iteration_ms_median=med,
        ratio_to_none={k: round(v / med["none"], 4) for k, v in med.items()} if "none" in med else {}, **info)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
