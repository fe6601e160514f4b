"""What extrinsic priors cost at run time: a `pose` prior on every free extrinsic against no priors,
on one handle per problem and solver.

  C3 (1k cameras, 1M observations): the EXPLICIT and the PCG LM iteration;
  C5 (rig 16 x 64, 10M observations): the EXPLICIT and the mixed-precision PCG LM iteration
     (--no-c5 skips it).
Convention: a warmed handle, then --reps solves of up to --lm-iters LM iterations from the same
start with all tolerances 0, without and with priors in turn; per solve the median host wall-clock
per LM iteration. Prints one JSON line. The expectation from the code is two small launches per
iteration (k_prior_blocks after each evaluation pass, k_prior_candidate after each candidate pass).
--trace-only runs one C3 EXPLICIT solve with priors and nothing else (for a kernel trace).
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


def pose_priors(prob, seed=11):
    """A = Q D (I + 0.2 G), D = diag(1/0.02 x3, 1/0.05 x3), mean = start + sigma o normal, on every
    non-constant extrinsic (tests/prior_ref.py's `pose`)."""
    rng = np.random.default_rng(seed)
    sig = np.array([0.02] * 3 + [0.05] * 3)
    idx = np.flatnonzero(prob.ext_const == 0).astype(np.int32)
    A, mu = [], []
    for e in idx:
        Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
        G = rng.standard_normal((6, 6))
        A.append(Q @ np.diag(1.0 / sig) @ (np.eye(6) + 0.2 * G))
        mu.append(prob.ext[e] + sig * rng.standard_normal(6))
    return idx, np.array(mu), np.array(A)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lm-iters", type=int, default=10)
    ap.add_argument("--no-c5", action="store_true")
    ap.add_argument("--trace-only", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (the GPU runtime is initialised before libdab loads)
    torch.cuda.is_available()
    import _pkgload
    pkg = _pkgload.load()
    tol0 = dict(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=0.0)
    E, P = pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG
    runs = [("c3_explicit", "c3_1kcam", dict(linear_solver_type=E)), ("c3_pcg", "c3_1kcam", dict(linear_solver_type=P))]
    if not a.no_c5:
        runs += [("c5_explicit", "c5_rig_16x64", dict(linear_solver_type=E)),
                 ("c5_pcg_fp32", "c5_rig_16x64", dict(linear_solver_type=P, pcg_fp32=1))]
    if a.trace_only:
        runs = runs[:1]
    out = {}
    probs = {}
    for name, cfg, kw in runs:
        if cfg not in probs:
            probs.clear()
            probs[cfg] = pkg.synth(**pkg.CONFIGS[cfg])
        prob = probs[cfg].copy()
        start = prob.copy()
        priors = pose_priors(start)
        opts = pkg.options(max_num_iterations=a.lm_iters, **tol0, **kw)
        s = pkg.Solver(0)
        s.set_problem(prob)
        rec = {"none": [], "pose": []}
        info = {}
        for rep in range(1 if a.trace_only else a.reps + 1):  # interleaved; the first round warms up
            for which in (("pose",) if a.trace_only else ("none", "pose")):
                s.set_ext_priors(*priors) if which == "pose" else s.set_ext_priors(None)
                s.update_parameters(start.points, start.ext)
                r = s.solve(opts)
                if rep or a.trace_only:
                    rec[which].append(round(median_iteration_ms(r), 4))
                    info[which] = dict(iterations=r["num_iterations"], rejected=r["num_unsuccessful_steps"],
                                       num_residuals=r["num_residuals"], initial_cost=r["initial_cost"],
                                       final_cost=r["final_cost"], schur_assembly=r["schur_assembly"],
                                       cg=[it["linear_solver_iterations"] for it in r["iterations"]])
        s.close()
        out[name] = dict(lm_iteration_ms=rec, num_priors=int(len(priors[0])),
                         lm_iteration_ms_median={k: float(np.median(v)) for k, v in rec.items() if v}, **info)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
