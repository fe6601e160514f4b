"""What point priors cost at run time: no priors, a prior on 100 points and a prior on every point,
on one handle per problem and solver (the sibling of scripts/prior_cost.py).

  C3 (1k cameras, 1M observations): the EXPLICIT and the PCG LM iteration;
  C5 (rig 16 x 64, 10M observations, 1M points): the EXPLICIT and the mixed-precision PCG LM
     iteration (--no-c5 skips it).
Convention (prior_cost.py's): a warmed handle, then --reps solves of up to --lm-iters LM iterations
from the same start with all tolerances 0, the three variants in turn; per solve the median host
wall-clock per LM iteration. Prints one JSON line. The expectation from the byte counts: 144 B of
records and 144 B of V | g read-modify-write per prior and evaluation (k_pt_prior_blocks), 96 B of
records and 72 B of points and step per prior and candidate pass (k_pt_prior_candidate): with a
prior on each of a million points about 0.5 GB per accepted iteration, 0.1 ms at HBM rates.
--trace-only runs one C5 EXPLICIT solve with a prior on every point and nothing else (for a kernel
trace).
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


def point_priors(prob, idx, seed=11):
    """A = Q D (I + 0.2 G), D = diag(1 / (0.1, 0.01, 0.001)), mean = start + 2 sigma o normal
    (tests/ptprior_ref.py's `all`, drawn in one batch) on the points idx."""
    rng = np.random.default_rng(seed)
    sig = np.array([0.1, 0.01, 0.001])
    n = len(idx)
    Q, _ = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    A = Q @ (np.diag(1.0 / sig) @ (np.eye(3) + 0.2 * rng.standard_normal((n, 3, 3))))
    return idx.astype(np.int32), prob.points[idx] + 2.0 * sig * rng.standard_normal((n, 3)), A


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
        runs = [("c5_explicit", "c5_rig_16x64", dict(linear_solver_type=E))]
    variants = ("every",) if a.trace_only else ("none", "p100", "every")
    out = {}
    probs = {}
    for name, cfg, kw in runs:
        if cfg not in probs:
            probs.clear()
            probs[cfg] = pkg.synth(**pkg.CONFIGS[cfg])
        prob = probs[cfg].copy()
        start = prob.copy()
        ref = np.unique(start.obs_point)
        sets = {"none": None, "p100": point_priors(start, ref[np.linspace(0, len(ref) - 1, 100).astype(np.int64)]),
                "every": point_priors(start, ref)}
        opts = pkg.options(max_num_iterations=a.lm_iters, **tol0, **kw)
        s = pkg.Solver(0)
        s.set_problem(prob)
        rec = {v: [] for v in variants}
        info = {}
        for rep in range(1 if a.trace_only else a.reps + 1):  # interleaved; the first round warms up
            for which in variants:
                s.set_point_priors(*sets[which]) if sets[which] is not None else s.set_point_priors(None)
                s.update_parameters(start.points, start.ext)
                r = s.solve(opts)
                if rep or a.trace_only:
                    rec[which].append(round(median_iteration_ms(r), 4))
                    info[which] = dict(iterations=r["num_iterations"], rejected=r["num_unsuccessful_steps"],
                                       num_residuals=r["num_residuals"], initial_cost=r["initial_cost"],
                                       final_cost=r["final_cost"], schur_assembly=r["schur_assembly"],
                                       cg=[it["linear_solver_iterations"] for it in r["iterations"]])
        s.close()
        med = {k: float(np.median(v)) for k, v in rec.items() if v}
        out[name] = dict(lm_iteration_ms=rec, num_points=int(len(ref)), lm_iteration_ms_median=med,
                         ratio_to_none={k: round(v / med["none"], 4) for k, v in med.items()} if "none" in med else {},
                         **info)
        print(name, out[name]["lm_iteration_ms_median"], file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
