"""What the cross-block kernels of dab_covariance_blocks cost beside the point blocks' fold-back.

usage: python scripts/cov_blocks_cost.py --config c3|c5 [--calls N]
One handle, one warm call per list, then the median over --calls calls of blocks_ms (the device
time of k_covx_pp / k_covx_pc, HIP events inside the call) and of info.points_ms of the same call
(k_cov_merge, k_cov_gz with free intrinsics, k_cov_points):
  c3 (1k cameras, 100k points, one more constant extrinsic: full rank)
     pe: the (point, extrinsic) pair of every observation (1M)
     pp: 100k random pairs of points
  c5 (the 16 x 64 rig, 1M points, every group of every intrinsic free)
     pz: 1M pairs (point, the intrinsic of its first observation)
with the gathers each list makes (6x6 blocks of C, 288 B each): sum over the pairs of k(p) for pe /
pz and of k(p) k(p') for pp, against sum over the points of k (k + 1) / 2 for the point blocks
(k: the records of a point, its distinct free cameras plus the free intrinsics it sees).
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def records_per_point(prob, with_intr):
    const = prob.ext_const.astype(bool)
    ne = prob.ext.shape[0]
    m1 = prob.obs_ext1 >= 0
    pt = np.concatenate([prob.obs_point, prob.obs_point[m1]]).astype(np.int64)
    ex = np.concatenate([prob.obs_ext0, prob.obs_ext1[m1]]).astype(np.int64)
    pairs = np.unique((pt * ne + ex)[~const[ex]])
    k = np.bincount(pairs // ne, minlength=prob.points.shape[0]).astype(np.int64)
    if with_intr:
        ni = prob.intr.shape[0]
        zp = np.unique(prob.obs_point.astype(np.int64) * ni + prob.obs_intr)
        k += np.bincount(zp // ni, minlength=prob.points.shape[0])
    return k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=("c3", "c5"))
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    import torch  # noqa: F401  (the GPU runtime is initialised before libdab loads)
    torch.cuda.is_available()
    import _pkgload
    pkg = _pkgload.load()
    name = {"c3": "c3_1kcam", "c5": "c5_rig_16x64"}[a.config]
    prob = pkg.synth(**pkg.CONFIGS[name])
    prob.ext_const[1] = 1  # beside extrinsic 0 (the gauge rule): fixes the scale
    rng = np.random.default_rng(1)
    npts = prob.points.shape[0]
    k = records_per_point(prob, a.config == "c5")
    lists = {}
    if a.config == "c3":
        lists["pe"] = np.stack([prob.obs_point, prob.obs_ext0], axis=1).astype(np.int32)
        lists["pp"] = rng.integers(0, npts, (100000, 2)).astype(np.int32)
    else:
        first = np.full(npts, -1, np.int64)
        first[prob.obs_point[::-1]] = prob.obs_intr[::-1]
        p = rng.integers(0, npts, 1000000)
        p = p[first[p] >= 0]
        lists["pz"] = np.stack([p, first[p]], axis=1).astype(np.int32)
    s = pkg.Solver(0)
    s.set_problem(prob)
    if a.config == "c5":
        s.set_intrinsics_free(7)
    out = dict(config=name, calls=a.calls, point_block_gathers=int((k * (k + 1) // 2).sum()))
    for kind, lst in lists.items():
        rows = []
        for _ in range(a.calls + 1):
            g = s.covariance_blocks(**{kind: lst})
            assert g["info"]["status"] == "OK", g["info"]
            assert np.isfinite(g[kind]).all()
            rows.append(g["info"])
        if kind == "pp":
            gathers = int((k[lst[:, 0]] * k[lst[:, 1]]).sum())
        elif kind == "pe":
            gathers = int(k[lst[:, 0]][~prob.ext_const.astype(bool)[lst[:, 1]]].sum())
        else:
            gathers = int(k[lst[:, 0]].sum())
        b = [r["blocks_ms"] for r in rows[1:]]
        q = [r["points_ms"] for r in rows[1:]]
        out[kind] = dict(pairs=int(len(lst)), gathers=gathers, blocks_ms=[round(x, 4) for x in b],
                         points_ms=[round(x, 4) for x in q], blocks_ms_median=round(float(np.median(b)), 4),
                         points_ms_median=round(float(np.median(q)), 4),
                         ratio=round(float(np.median(b) / np.median(q)), 3),
                         gather_ratio=round(gathers / max(1, out["point_block_gathers"]), 3),
                         gather_gb_per_s=round(288.0 * gathers / (1e-3 * float(np.median(b))) / 1e9, 1))
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
