"""What dab_covariance costs, and that it leaves dab_solve alone.

Driver (no arguments): runs every measurement below in a child process of its own under a
time limit, stops at the first child that fails, and writes profiles/r08_covariance.json.
  * covariance stage times (evaluate / factor / inverse / points, HIP events inside the call) at
    C2, C3 and C5 with one more constant extrinsic (full rank): median of --calls calls after one
    warm call, with n, inverse_ms / factor_ms and the point kernel's gathered bytes / time
    (k (k + 1) / 2 blocks of 288 B per point of k distinct free cameras);
  * the exact LM iteration (median over a --lm-iters solve) at C3 and C5 with this tree's library
    and, with --parent-lib PATH (a libdab.so built from the parent commit), with the parent's, in
    interleaved pairs: this, parent, this, parent, ...
Child: --child cov|lm --config NAME [--lib PATH] prints one JSON line.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": "c2_100cam", "c3": "c3_1kcam", "c5": "c5_rig_16x64"}


def load_pkg(lib):
    import torch  # noqa: F401  (the GPU runtime is initialised before libdab loads)
    torch.cuda.is_available()
    import _pkgload
    pkg = _pkgload.load()
    if lib:  # another build of the library (the parent commit's: it has no covariance symbols)
        abi = sys.modules[pkg.__name__ + "._abi"]
        abi.LIB_PATH = os.path.abspath(lib)
        for k in [k for k in abi.SIGNATURES if "covariance" in k]:
            del abi.SIGNATURES[k]
    return pkg


def full_rank(pkg, name):
    prob = pkg.synth(**pkg.CONFIGS[CONFIGS[name]])
    prob.ext_const[1] = 1  # beside extrinsic 0 (the gauge rule): fixes the scale
    return prob


def child_cov(a):
    pkg = load_pkg(a.lib)
    prob = full_rank(pkg, a.config)
    const = prob.ext_const.astype(bool)
    m1 = prob.obs_ext1 >= 0
    pt = np.concatenate([prob.obs_point, prob.obs_point[m1]]).astype(np.int64)
    ex = np.concatenate([prob.obs_ext0, prob.obs_ext1[m1]]).astype(np.int64)
    pairs = np.unique((pt * prob.ext.shape[0] + ex)[~const[ex]])  # distinct (point, free camera)
    k = np.bincount(pairs // prob.ext.shape[0], minlength=prob.points.shape[0]).astype(float)
    gathered = float((k * (k + 1) / 2).sum() * 288.0)
    s = pkg.Solver(0)
    s.set_problem(prob)
    rows = []
    for _ in range(a.calls + 1):
        rows.append(s.covariance(points=True, ext=True, full=False)["info"])
    s.close()
    assert all(r["status"] == "OK" for r in rows), rows[0]
    med = {f: float(np.median([r[f] for r in rows[1:]])) for f in ("evaluate_ms", "factor_ms", "inverse_ms", "points_ms")}
    out = dict(config=CONFIGS[a.config], n=6 * rows[0]["num_free_ext"], points=int(rows[0]["num_free_points"]),
               schur_assembly=rows[0]["schur_assembly"], calls=a.calls, **{f: round(v, 4) for f, v in med.items()},
               inverse_over_factor=round(med["inverse_ms"] / med["factor_ms"], 3),
               point_gather_bytes=gathered,
               point_gather_gb_per_s=round(gathered / (1e-3 * med["points_ms"]) / 1e9, 2),
               camera_pivot_ratio=rows[0]["camera_pivot_ratio"], point_pivot_ratio_min=rows[0]["point_pivot_ratio_min"])
    print(json.dumps(out))


def child_lm(a):
    pkg = load_pkg(a.lib)
    prob = pkg.synth(**pkg.CONFIGS[CONFIGS[a.config]])
    s = pkg.Solver(0)
    s.set_problem(prob)
    r = s.solve(pkg.options(max_num_iterations=a.lm_iters, linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR))
    s.close()
    t = [it["time"] for it in r["iterations"][1:]]
    print(json.dumps(dict(config=CONFIGS[a.config], lm_iteration_ms=round(1e3 * float(np.median(t)), 4),
                          iterations=len(t), final_cost=r["final_cost"])))


def run_child(args, limit):
    """One GPU step in a process of its own under a time limit; None when it failed."""
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        sys.stderr.write(f"cov_cost: {' '.join(args)} ran past {limit} s\n")
        return None
    if p.returncode != 0:
        sys.stderr.write(f"cov_cost: {' '.join(args)} failed ({p.returncode})\n{p.stderr[-2000:]}\n")
        return None
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--config", default="c2")
    ap.add_argument("--lib", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--lm-iters", type=int, default=6)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--configs", default="c2,c3,c5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_covariance.json"))
    a = ap.parse_args()
    if a.child == "cov":
        return child_cov(a)
    if a.child == "lm":
        return child_lm(a)
    out = dict(what="dab_covariance: stage times (HIP events inside the call, median of the calls after a warm "
               "one) and the exact LM iteration with and without the feature in the library",
               covariance={}, lm_iteration_ms={})

    def save():
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for name in a.configs.split(","):
        r = run_child(["--child", "cov", "--config", name, "--calls", str(a.calls)], 420)
        if r is None:
            save()
            return 1
        out["covariance"][name] = r
        save()
    for name in [n for n in a.configs.split(",") if n in ("c3", "c5")]:
        rows = out["lm_iteration_ms"][name] = dict(this=[], parent=[])
        for _ in range(a.pairs):
            for who, lib in (("this", ""), ("parent", a.parent_lib)):
                if who == "parent" and not a.parent_lib:
                    continue
                r = run_child(["--child", "lm", "--config", name, "--lm-iters", str(a.lm_iters)] +
                              (["--lib", lib] if lib else []), 300)
                if r is None:
                    save()
                    return 1
                rows[who].append(r["lm_iteration_ms"])
                save()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main() or 0)
