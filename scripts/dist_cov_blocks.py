"""Two-rank check of dab_covariance_blocks with the host-staged collective on one GPU.

Launch: python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1
        --master-port P scripts/dist_cov_blocks.py --device D [--tol T]
bal40 (cameras 0 and 1 constant) with its first 16 intrinsics free, split by point. Every rank
asks its shard's handle for the same lists over all global points: one pp pair per point (with the
next point), its pe pair with two extrinsics, its pz pair with one free and one constant
intrinsic. Rank 0 asks a single handle on the whole problem for the same lists and checks:
  - a block whose points all belong to the rank is within T max |Sigma| of the single handle's
    (T = 64 kappa 2^-53 from the caller; max |Sigma| over the single handle's cam_full and
    point_cov), exact zeros are zeros on both;
  - a block naming a point of the other rank is NaN.
Prints DIST_COV_BLOCKS OK or FAIL."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tol", type=float, default=1e-9)
    a = ap.parse_args()
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    import torch
    import torch.distributed as dist

    import _pkgload

    pkg = _pkgload.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)

    def gloo_allreduce(arr, op):
        t = torch.from_numpy(arr)
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM)

    glob = pkg.synth(kind=0, num_cameras=40, num_points=200, obs_per_point=8, seed=5)
    glob.ext_const[1] = 1
    groups = np.zeros(glob.intr.shape[0], np.uint8)
    groups[:16] = 7
    npts, next_ = glob.points.shape[0], glob.ext.shape[0]
    owner = glob.point_owner(world)
    p = np.arange(npts)
    pp = np.stack([p, (p + 1) % npts], axis=1)
    pe = np.concatenate([np.stack([p, 2 + p % (next_ - 2)], axis=1), np.stack([p, (7 * p) % next_], axis=1)])
    pz = np.concatenate([np.stack([p, p % 16], axis=1), np.stack([p, 16 + p % 24], axis=1)])
    lists = dict(pp=pp.astype(np.int32), pe=pe.astype(np.int32), pz=pz.astype(np.int32))
    # which rank can answer each pair (-1: none, its points belong to different ranks)
    who = dict(pp=np.where(owner[pp[:, 0]] == owner[pp[:, 1]], owner[pp[:, 0]], -1), pe=owner[pe[:, 0]],
               pz=owner[pz[:, 0]])

    s = pkg.Solver(a.device, rank, world, None, host_allreduce=gloo_allreduce)
    s.set_problem(glob.copy().shard(rank, world))
    s.set_intrinsics_free(groups)
    g = s.covariance_blocks(**lists)
    s.close()
    ok_here = g["info"]["status"] == "OK"
    nan_ok = ok_here and all(np.isnan(g[k][who[k] != rank]).all() and not np.isnan(g[k][who[k] == rank]).any()
                             for k in lists)
    flags = torch.tensor([1 if ok_here else 0, 1 if nan_ok else 0], dtype=torch.int32)
    dist.all_reduce(flags)
    mine = {}
    for k in lists:
        blk = g[k] if ok_here else np.zeros((len(lists[k]), 3, 3 if k == "pp" else 6))
        t = torch.from_numpy(np.where((who[k] == rank)[:, None, None], blk, 0.0))
        dist.all_reduce(t)
        mine[k] = t.numpy()
    if rank == 0:
        s1 = pkg.Solver(a.device)
        s1.set_problem(glob.copy())
        s1.set_intrinsics_free(groups)
        g1 = s1.covariance_blocks(**lists)
        c1 = s1.covariance(full=True, intrinsics=True)
        s1.close()
        res = dict(ranks_ok=int(flags[0]), nan_ok=int(flags[1]), single=g1["info"]["status"])
        good = res["ranks_ok"] == world and res["nan_ok"] == world and res["single"] == "OK"
        if good:
            m = max(float(np.abs(c1["cam_full"]).max()), float(np.nanmax(np.abs(c1["point_cov"]))))
            res.update(m=m, tol=a.tol * m)
            for k in lists:
                ans = who[k] >= 0
                res[k + "_err"] = float(np.abs(mine[k][ans] - g1[k][ans]).max())
                res[k + "_answered"] = int(ans.sum())
                good = good and res[k + "_err"] <= a.tol * m and res[k + "_answered"] > 0
                good = good and bool(((g1[k][ans] == 0.0) == (mine[k][ans] == 0.0)).all())
            good = good and int((who["pp"] < 0).sum()) > 0
        print(json.dumps(res, indent=1))
        sys.stdout.write("DIST_COV_BLOCKS " + ("OK" if good else "FAIL") + "\n")
        sys.stdout.flush()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
