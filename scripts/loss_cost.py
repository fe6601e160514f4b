"""What a robust loss costs at run time: Cauchy(0.5) against the TRIVIAL loss on one handle.

  C3 (1k cameras, 1M observations): the evaluation pass (us per pass over a batch, and the
     sampled kernel times), and the PCG LM iteration;
  C5 (rig 16 x 64, 10M observations): the EXPLICIT LM iteration (--no-c5 skips it).
Prints one JSON line. The expectation is one reciprocal and one square root more per
observation in every pass that evaluates rows (and a logarithm where the cost is formed).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_iteration_ms(summary):
    t = [it["time"] for it in summary["iterations"][1:]]
    return 1e3 * float(np.median(t)) if t else float("nan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lm-iters", type=int, default=6)
    ap.add_argument("--no-c5", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401  (the GPU runtime is initialised before libdab loads)
    torch.cuda.is_available()
    import _pkgload
    pkg = _pkgload.load()
    losses = (("trivial", 1.0), ("cauchy", 0.5))
    out = {}

    prob = pkg.synth(**pkg.CONFIGS["c3_1kcam"])
    start = prob.copy()
    s = pkg.Solver(0)
    s.set_problem(prob)
    ev = {k: [] for k, _ in losses}
    km = {}
    for rep in range(a.reps + 1):  # interleaved; the first round warms up
        for kind, scale in losses:
            s.set_loss(kind, scale)
            s.bench_eval_pass(True, 20)
            s.sync()
            s.bench_kernel_ms()
            t0 = time.perf_counter()
            s.bench_eval_pass(True, a.steps)
            s.sync()
            dt = time.perf_counter() - t0
            if rep:
                ev[kind].append(1e6 * dt / a.steps)
                km[kind] = s.bench_kernel_ms()
    out["c3_eval_pass_us"] = {k: [round(x, 2) for x in v] for k, v in ev.items()}
    out["c3_eval_kernel_ms"] = {k: [round(x, 5) for x in v] for k, v in km.items()}
    lm = {k: [] for k, _ in losses}
    opts = pkg.options(max_num_iterations=a.lm_iters, linear_solver_type=pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG)
    for rep in range(a.reps + 1):
        for kind, scale in losses:
            s.set_loss(kind, scale)
            s.update_parameters(start.points, start.ext)
            r = s.solve(opts)
            if rep:
                lm[kind].append(round(median_iteration_ms(r), 4))
                out.setdefault("c3_pcg_cg_iterations", {})[kind] = [it["linear_solver_iterations"]
                                                                   for it in r["iterations"]]
    out["c3_pcg_lm_iteration_ms"] = lm
    s.close()

    if not a.no_c5:
        prob = pkg.synth(**pkg.CONFIGS["c5_rig_16x64"])
        start = prob.copy()
        s = pkg.Solver(0)
        s.set_problem(prob)
        lm = {k: [] for k, _ in losses}
        opts = pkg.options(max_num_iterations=a.lm_iters, linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)
        for rep in range(a.reps + 1):
            for kind, scale in losses:
                s.set_loss(kind, scale)
                s.update_parameters(start.points, start.ext)
                r = s.solve(opts)
                if rep:
                    lm[kind].append(round(median_iteration_ms(r), 4))
        out["c5_explicit_lm_iteration_ms"] = lm
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
