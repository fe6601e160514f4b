"""Multi-rank check of the RCCL path on whatever GPUs the box has.

Launch: python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1
        --master-port P scripts/dist_check.py [--device D]
Every rank solves its point shard of one global problem through dab_create_dist; rank 0
also solves the global problem on one handle and compares the LM trajectories (explicit
Schur and PCG). With --device D every rank uses device D (ranks sharing one GPU; RCCL
refuses that, so pair it with --host-collective, which stages the library's collectives
through gloo and exercises every other part of the sharded path). --loss kind:scale sets a
robust loss (dab_set_loss) on every rank's handle and on the single handle it is compared with.
--free-intrinsics G sets the DAB_INTR_* groups G free on every intrinsic (dab_set_intrinsics_free),
on every rank's handle and on the single handle; the refined intrinsics are compared too (the exact
step only: pair it with --solvers explicit).
--const-points third|all holds every third point (by global id), or every point, constant
(dab_set_points_constant) on every rank's shard and on the single handle; the constant points must
come back bitwise untouched, and with `all` every rank must report the direct camera step
(DAB_SCHUR_DIRECT) for the explicit and the AUTO solver (pair it with --solvers explicit,auto).
--ext-scalars rot-odd|trans-all|mix holds scalars of the extrinsics constant
(dab_set_ext_scalars_constant; the masks of tests/extsub_ref.py), the same on every rank's handle and
on the single handle; they must come back bitwise untouched on every rank.
--ext-priors pose sets a full Gaussian prior on every non-constant extrinsic (dab_set_ext_priors),
the same on every rank's handle and on the single handle: a prior added once per rank instead of
once shows as a cost difference far above --tol (the priors' share of the initial cost is printed
and must be above 100 --tol). Off by default.
--pt-priors all sets a full Gaussian prior on every point (dab_set_point_priors): all of them on the
single handle, on each rank those of the points it owns (Problem.shard_point_priors; every rank must
get at least one). A cost not summed over the ranks or a candidate term added after the sum shows
as a cost difference far above --tol (the priors' share of the initial cost is printed and must be
above 100 --tol). Off by default.
--intr-priors calib, with --free-intrinsics, sets a full Gaussian prior on every intrinsic
(dab_set_intr_priors: A = Q diag(1 / sigma) (I + 0.2 G), sigma = (2, 2, 5e-3 |f0|, 5e-3 |f1|, 5e-3,
5e-3), mean = start + sigma o normal), the same on every rank's handle and on the single handle:
intrinsics are replicated, so a prior added once per rank instead of once shows as a cost
difference far above --tol (the priors' share of the initial cost is printed and must be above
100 --tol). Off by default.
--expect-auto-refused checks instead that LINEAR_SOLVER_AUTO, where it picks PCG (several ranks, a
camera system that is not a small one), refuses a non-empty free set on every rank.
--covariance checks dab_covariance instead: every rank calls it on its shard after the solve, and
rank 0 compares the camera arrays across the ranks (bitwise) and, with every owner's point rows,
against a single handle at the same parameters. --cov-intrinsics K does the same for
dab_covariance_intrinsics with the first K intrinsics free.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=-1)
    ap.add_argument("--host-collective", action="store_true",
                    help="stage the library's all-reduces through gloo (ranks sharing a GPU)")
    ap.add_argument("--config", default="", help="a named configuration (core.CONFIGS) instead of "
                    "the small BAL and rig problems, e.g. c3_1kcam: BASELINE config 4's partition")
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--expect-p2p", action="store_true",
                    help="fail unless the one-shot peer-to-peer all-reduce carried the sums")
    ap.add_argument("--live-together", action="store_true",
                    help="keep the three sharded handles of a problem alive at once (bench.py holds two: "
                    "each takes its own slot of the peer-to-peer arena)")
    ap.add_argument("--expect-no-p2p", action="store_true",
                    help="fail if the peer-to-peer path is in use (its set-up self-test must have "
                    "failed over to the other collectives)")
    ap.add_argument("--solvers", default="explicit,pcg,auto",
                    help="comma list of the linear solvers to check (explicit, pcg, auto)")
    ap.add_argument("--tol", type=float, default=1e-8,
                    help="largest relative per-iteration cost difference against the single handle")
    ap.add_argument("--expect-cg-equal", action="store_true",
                    help="fail unless every iteration's CG count equals the single handle's")
    ap.add_argument("--expect-auto", default="",
                    help="fail unless AUTO ran this solver on the ranks (explicit | pcg)")
    ap.add_argument("--timeout-rank", type=int, default=-1,
                    help="this rank's evaluation pass runs a frame wait that never completes "
                    "(DAB_EVAL_SIDE=7): every rank's dab_solve must fail with the timeout, none may hang")
    ap.add_argument("--loss", default="", help="robust loss kind:scale (huber | soft_l1 | cauchy, e.g. "
                    "cauchy:0.5), set on every rank's handle and on the single-handle comparison")
    ap.add_argument("--free-intrinsics", type=int, default=0,
                    help="DAB_INTR_* group bits refined on every handle (every rank sets the same mask); the "
                    "result is compared with the single handle at --tol")
    ap.add_argument("--const-points", default="", choices=("", "third", "all"),
                    help="constant points on every handle: every third point by global id, or all of them (then "
                    "every rank must take the direct camera step, S = U + D^2, also under AUTO)")
    ap.add_argument("--ext-scalars", default="", choices=("", "rot-odd", "trans-all", "mix"),
                    help="constant scalars of the extrinsics, the same bits on every handle")
    ap.add_argument("--ext-priors", default="", choices=("", "pose"),
                    help="Gaussian priors on every non-constant extrinsic, the same on every handle")
    ap.add_argument("--pt-priors", default="", choices=("", "all"),
                    help="Gaussian priors on every point, split over the ranks with the points")
    ap.add_argument("--intr-priors", default="", choices=("", "calib"),
                    help="with --free-intrinsics: Gaussian priors on every intrinsic, the same on every handle")
    ap.add_argument("--expect-auto-refused", action="store_true",
                    help="with --free-intrinsics: a rig whose tables do not fit the small-camera paths (135 "
                    "extrinsics), so AUTO picks PCG on several ranks; every rank's dab_solve must return "
                    "DAB_E_UNSUPPORTED, leave the parameters alone, and solve with the mask cleared")
    ap.add_argument("--covariance", action="store_true",
                    help="after the solve (--iters LM iterations of the exact step; 0 = none) every rank calls "
                    "dab_covariance: the camera arrays must be bitwise equal across the ranks and, like every "
                    "owner's point rows, within --cov-tol of a single handle at the same parameters")
    ap.add_argument("--cov-tol", type=float, default=1e-9,
                    help="--covariance: bound on max |difference| / max |Sigma| against the single handle")
    ap.add_argument("--cov-intrinsics", type=int, default=0,
                    help="--covariance: the first K intrinsics are free (all groups, the same mask on every "
                    "handle) and the call is dab_covariance_intrinsics; the camera arrays compared are then "
                    "cam_full and the extrinsic blocks followed by the intrinsic ones")
    a = ap.parse_args()
    loss = None
    if a.loss:
        kind, _, scale = a.loss.partition(":")
        loss = (kind, float(scale) if scale else 1.0)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dev = a.device if a.device >= 0 else int(os.environ.get("LOCAL_RANK", "0"))
    import torch
    import torch.distributed as dist

    import _pkgload

    pkg = _pkgload.load()
    dist.init_process_group("gloo", rank=rank, world_size=world)
    buf = torch.zeros(128, dtype=torch.uint8)
    if rank == 0:
        buf[:] = torch.tensor(list(pkg.Solver.unique_id()), dtype=torch.uint8)
    dist.broadcast(buf, 0)
    uid = bytes(buf.tolist())
    def gloo_allreduce(arr, op):
        t = torch.from_numpy(arr)
        dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM)

    if a.timeout_rank >= 0:
        # one rank's pass times out inside the launch; its error word travels with the cost's
        # all-reduce, so every rank must fail the same call (DAB_E_DEVICE), none may hang
        if rank == a.timeout_rank:
            os.environ["DAB_EVAL_SIDE"] = "7"  # read when the handle is created
        glob = pkg.synth(**pkg.CONFIGS[a.config]) if a.config else \
            pkg.synth(kind=0, num_cameras=40, num_points=4000, obs_per_point=6, seed=61)
        s = pkg.Solver(dev, rank, world, uid, host_allreduce=gloo_allreduce if a.host_collective else None)
        msg = ""
        try:
            s.set_problem(glob.copy().shard(rank, world))
            sched = s.eval_fused()
            s.solve(pkg.options(max_num_iterations=3))
        except RuntimeError as e:
            msg = str(e)
        finally:
            s.close()
        failed = torch.tensor([1 if "timed out" in msg else 0], dtype=torch.int32)
        dist.all_reduce(failed)
        if rank == 0:
            ok = int(failed.item()) == world and sched == 2
            sys.stdout.write(f"DIST_CHECK {'OK' if ok else 'FAIL'} timeout: {int(failed.item())}/{world} ranks "
                             f"failed closed, eval schedule {sched}, rank 0: {msg!r}\n")
            sys.stdout.flush()
        dist.destroy_process_group()
        return

    if a.expect_auto_refused:
        # LINEAR_SOLVER_AUTO resolves to IMPLICIT_SCHUR_PCG only on several ranks and only when the
        # camera system is not a small one: the refusal of free intrinsics must then come from the
        # solver AUTO chose, on every rank, and leave the handle usable
        glob = pkg.synth(kind=1, num_arcs=16, num_rings=120, num_points=1500, obs_per_point=6, seed=63)
        mine = glob.copy().shard(rank, world)
        s = pkg.Solver(dev, rank, world, uid, host_allreduce=gloo_allreduce if a.host_collective else None)
        auto = pkg.options(max_num_iterations=3, linear_solver_type=pkg.DAB_LINEAR_SOLVER_AUTO)
        msg, after = "", None
        try:
            s.set_problem(mine)
            s.set_intrinsics_free(a.free_intrinsics or 7)
            nfi = s.get_intrinsics_free()[1]
            try:
                s.solve(auto)
            except RuntimeError as e:
                msg = str(e)
            untouched = (np.array_equal(mine.points, glob.points) and np.array_equal(mine.ext, glob.ext)
                         and np.array_equal(s.get_intrinsics(), glob.intr))
            s.set_intrinsics_free(None)
            after = s.solve(auto)
        finally:
            s.close()
        good = ("libdab error -6" in msg and "exact step" in msg and untouched and nfi == glob.intr.shape[0]
                and after["linear_solver_type_used"] == pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG
                and after["final_cost"] < after["initial_cost"])
        ok = torch.tensor([1 if good else 0], dtype=torch.int32)
        dist.all_reduce(ok)
        if rank == 0:
            sys.stdout.write(f"DIST_CHECK {'OK' if int(ok.item()) == world else 'FAIL'} auto refused: "
                             f"{int(ok.item())}/{world} ranks, {nfi} free intrinsics, {glob.ext.shape[0]} extrinsics, "
                             f"rank 0: {msg!r}, then solver {after['linear_solver_type_used']}\n")
            sys.stdout.flush()
        dist.destroy_process_group()
        return

    if a.covariance:
        def covariance_of(solver):
            """dab_covariance, or with --cov-intrinsics dab_covariance_intrinsics under the names of the former"""
            if a.cov_intrinsics <= 0:
                return solver.covariance(full=True)
            g = np.zeros(solver.problem.intr.shape[0], np.uint8)
            g[:a.cov_intrinsics] = 7
            solver.set_intrinsics_free(g)
            c = solver.covariance(full=True, intrinsics=True)
            c["info"]["num_free_ext"] += c["info"]["num_free_intr"]
            if c["info"]["status"] == "OK":
                c["ext_full"] = c["cam_full"]
                c["ext_cov"] = np.concatenate([c["ext_cov"], c["intr_cov"]])
            return c

        if a.config:
            glob = pkg.synth(**pkg.CONFIGS[a.config])
        else:  # 40 cameras, two of them constant: the scale gauge is fixed, J has full rank
            glob = pkg.synth(kind=0, num_cameras=40, num_points=200, obs_per_point=8, seed=5)
        glob.ext_const[1] = 1
        owner = glob.point_owner(world)
        mine = glob.copy().shard(rank, world)
        s = pkg.Solver(dev, rank, world, uid, host_allreduce=gloo_allreduce if a.host_collective else None)
        if loss:
            s.set_loss(*loss)
        s.set_problem(mine)
        if a.iters > 0:
            s.solve(pkg.options(max_num_iterations=a.iters, linear_solver_type=pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR))
        cov = covariance_of(s)
        s.close()
        ok_here = cov["info"]["status"] == "OK"
        status = torch.tensor([1 if ok_here else 0], dtype=torch.int32)
        dist.all_reduce(status)
        nfe = cov["info"]["num_free_ext"]
        own = (owner == rank)
        pts = torch.from_numpy(np.where(own[:, None], mine.points, 0.0))
        dist.all_reduce(pts)
        full = cov["ext_full"] if ok_here else np.zeros((6 * nfe, 6 * nfe))
        blocks = cov["ext_cov"] if ok_here else np.zeros((nfe, 6, 6))
        hi, lo = torch.from_numpy(full.copy()), torch.from_numpy(full.copy())
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        bhi, blo = torch.from_numpy(blocks.copy()), torch.from_numpy(blocks.copy())
        dist.all_reduce(bhi, op=dist.ReduceOp.MAX)
        dist.all_reduce(blo, op=dist.ReduceOp.MIN)
        pc = cov["point_cov"] if ok_here else np.zeros((glob.points.shape[0], 3, 3))
        pc = torch.from_numpy(np.where(own[:, None, None], pc, 0.0))  # every owner's rows (the others' are NaN)
        dist.all_reduce(pc)
        if rank == 0:
            g1 = glob.copy()
            g1.points[:] = pts.numpy()
            g1.ext[:] = mine.ext
            s1 = pkg.Solver(dev)
            if loss:
                s1.set_loss(*loss)
            s1.set_problem(g1)
            c1 = covariance_of(s1)
            s1.close()
            res = dict(ranks_ok=int(status.item()), single=c1["info"]["status"],
                       ranks_equal=bool(torch.equal(hi, lo) and torch.equal(bhi, blo)))
            good = res["ranks_ok"] == world and res["single"] == "OK" and res["ranks_equal"]
            if good:
                m = max(float(np.abs(c1["ext_full"]).max()), float(np.abs(c1["point_cov"]).max()))
                res.update(m=m, ext_full_err=float(np.abs(hi.numpy() - c1["ext_full"]).max()),
                           ext_cov_err=float(np.abs(bhi.numpy() - c1["ext_cov"]).max()),
                           point_cov_err=float(np.abs(pc.numpy() - c1["point_cov"]).max()), tol=a.cov_tol * m)
                good = max(res["ext_full_err"], res["ext_cov_err"], res["point_cov_err"]) <= a.cov_tol * m
            print(json.dumps(res, indent=1))
            sys.stdout.write("DIST_CHECK " + ("OK" if good else "FAIL covariance") + "\n")
            sys.stdout.flush()
        dist.destroy_process_group()
        return

    names = {"explicit": pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR, "pcg": pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG,
             "auto": pkg.DAB_LINEAR_SOLVER_AUTO}
    solvers = [names[x] for x in a.solvers.split(",")]
    out = {}
    # free intrinsics: the rig only (the small BAL problem has 40 per-camera intrinsics, more than
    # the 16 the exact step's border takes)
    for kind in ((a.config,) if a.config else ("rig",) if a.free_intrinsics else ("bal", "rig")):
        if kind == "bal":
            glob = pkg.synth(kind=0, num_cameras=40, num_points=4000, obs_per_point=6, seed=61)
        elif kind == "rig":
            glob = pkg.synth(kind=1, num_arcs=5, num_rings=12, num_points=3000, obs_per_point=7, seed=62)
        else:
            glob = pkg.synth(**pkg.CONFIGS[kind])
        owner = glob.point_owner(world)
        cmask = None
        if a.const_points:
            cmask = np.ones(glob.points.shape[0], bool)
            if a.const_points == "third":
                cmask = np.arange(glob.points.shape[0]) % 3 == 0
        ebits = None
        if a.ext_scalars:
            e = np.arange(glob.ext.shape[0])
            ebits = {"rot-odd": np.where(e % 2 == 1, 7, 0), "trans-all": np.full(e.shape, 56),
                     "mix": (37 * e + 11) & 63}[a.ext_scalars].astype(np.uint8)
            eheld = ((ebits[:, None] >> np.arange(6)) & 1).astype(bool)
        priors = None
        if a.ext_priors:
            # A = Q D (I + 0.2 G), D = diag(1/0.02 x3, 1/0.05 x3); mean = start + sigma o normal
            rng = np.random.default_rng(11)
            sig = np.array([0.02] * 3 + [0.05] * 3)
            pidx = np.flatnonzero(glob.ext_const == 0).astype(np.int32)
            pa = np.stack([np.linalg.qr(rng.standard_normal((6, 6)))[0] @ np.diag(1.0 / sig)
                           @ (np.eye(6) + 0.2 * rng.standard_normal((6, 6))) for _ in pidx])
            priors = (pidx, glob.ext[pidx] + sig * rng.standard_normal((len(pidx), 6)), pa)
        pt_priors = None
        if a.pt_priors:
            # A = Q D (I + 0.2 G), D = diag(1 / (0.1, 0.01, 0.001)); mean = start + 2 sigma o normal
            rng = np.random.default_rng(11)
            sig = np.array([0.1, 0.01, 0.001])
            qidx = np.arange(glob.points.shape[0], dtype=np.int32)
            qa = np.stack([np.linalg.qr(rng.standard_normal((3, 3)))[0] @ np.diag(1.0 / sig)
                           @ (np.eye(3) + 0.2 * rng.standard_normal((3, 3))) for _ in qidx])
            pt_priors = (qidx, glob.points + 2.0 * sig * rng.standard_normal((len(qidx), 3)), qa)
        intr_priors = None
        if a.intr_priors:
            if not a.free_intrinsics:
                raise SystemExit("--intr-priors needs --free-intrinsics")
            rng = np.random.default_rng(11)
            zidx = np.arange(glob.intr.shape[0], dtype=np.int32)
            za, zmu = [], []
            for k6 in glob.intr:
                sig = np.array([2.0, 2.0, 5e-3 * abs(k6[2]), 5e-3 * abs(k6[3]), 5e-3, 5e-3])
                sig[sig == 0.0] = 1.0
                q = np.linalg.qr(rng.standard_normal((6, 6)))[0]
                za.append(q @ np.diag(1.0 / sig) @ (np.eye(6) + 0.2 * rng.standard_normal((6, 6))))
                zmu.append(k6 + sig * rng.standard_normal(6))
            intr_priors = (zidx, np.array(zmu), np.array(za))
        prior_share = 0.0
        pt_prior_share = 0.0
        intr_prior_share = 0.0
        intr_eff = (0, 0)
        pt_eff = (0, 0)
        live = []
        if a.live_together:  # every handle of this problem created (and its arena slot taken) up front
            for _ in range(3):
                h = pkg.Solver(dev, rank, world, uid, host_allreduce=gloo_allreduce if a.host_collective else None)
                if loss:
                    h.set_loss(*loss)
                live.append(h)
        for li, lst in enumerate(solvers):
            opts = pkg.options(max_num_iterations=a.iters, linear_solver_type=lst)
            ref = None
            if rank == 0:
                g1 = glob.copy()
                s1 = pkg.Solver(dev)
                if loss:
                    s1.set_loss(*loss)
                s1.set_problem(g1)
                if a.free_intrinsics:
                    s1.set_intrinsics_free(a.free_intrinsics)
                if cmask is not None:
                    s1.set_points_constant(cmask)
                if ebits is not None:
                    s1.set_ext_scalars_constant(ebits)
                    assert s1.get_ext_scalars_constant()[1] > 0
                if priors is not None:
                    s1.set_ext_priors(*priors)
                    assert s1.get_ext_priors()[3] == len(priors[0])
                    prior_share = s1.eval_ext_priors()[1]
                if pt_priors is not None:
                    s1.set_point_priors(*pt_priors)
                    pt_prior_share = s1.eval_point_priors()[1]
                if intr_priors is not None:
                    s1.set_intr_priors(*intr_priors)
                    intr_prior_share = s1.eval_intr_priors()[1]
                ropts = opts
                if lst == pkg.DAB_LINEAR_SOLVER_AUTO:
                    # what AUTO must pick on several ranks: the exact step for small camera
                    # systems (the rig), PCG for large ones (BAL / config 4)
                    want = (pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR
                            if glob.ext.shape[0] <= 160 or a.const_points == "all" else pkg.DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG)
                    ropts = pkg.options(max_num_iterations=a.iters, linear_solver_type=want)
                ref = (s1.solve(ropts), g1.points.copy(), g1.ext.copy(), g1.intr.copy())
                prior_share /= ref[0]["initial_cost"]
                pt_prior_share /= ref[0]["initial_cost"]
                intr_prior_share /= ref[0]["initial_cost"]
                s1.close()
            dist.barrier()
            mine = glob.copy().shard(rank, world)
            s = live[li] if live else pkg.Solver(dev, rank, world, uid,
                                                 host_allreduce=gloo_allreduce if a.host_collective else None)
            if loss and not live:
                s.set_loss(*loss)  # the same loss on every rank (include/dab.h)
            s.set_problem(mine)
            if a.free_intrinsics:
                s.set_intrinsics_free(a.free_intrinsics)  # the same mask on every rank (include/dab.h)
            if cmask is not None:
                s.set_points_constant(cmask)  # the shard's points are the ones this rank references
            if ebits is not None:
                s.set_ext_scalars_constant(ebits)  # the same bits on every rank (include/dab.h)
            if priors is not None:
                s.set_ext_priors(*priors)  # the same priors on every rank (include/dab.h)
            if pt_priors is not None:
                s.set_point_priors(*glob.shard_point_priors(pt_priors, rank, world))  # this rank's points' priors
                pt_eff = (s.get_point_priors()[3], len(pt_priors[0]))
            if intr_priors is not None:
                s.set_intr_priors(*intr_priors)  # the same priors on every rank (include/dab.h)
                intr_eff = (s.get_intr_priors()[3], len(intr_priors[0]))
            sched = s.eval_fused()
            p2p = s.comm_p2p()
            summ = s.solve(opts)
            if not live:
                s.close()
            pts = torch.from_numpy(np.where((owner == rank)[:, None], mine.points, 0.0))
            dist.all_reduce(pts)
            ext = torch.from_numpy(mine.ext.copy())
            dist.all_reduce(ext, op=dist.ReduceOp.MAX)
            ext_min = torch.from_numpy(mine.ext.copy())
            dist.all_reduce(ext_min, op=dist.ReduceOp.MIN)
            kk = torch.from_numpy(mine.intr.copy())
            dist.all_reduce(kk, op=dist.ReduceOp.MAX)
            kk_min = torch.from_numpy(mine.intr.copy())
            dist.all_reduce(kk_min, op=dist.ReduceOp.MIN)
            asm = torch.tensor([summ["schur_assembly"], -summ["schur_assembly"]], dtype=torch.int32)
            dist.all_reduce(asm, op=dist.ReduceOp.MAX)  # (max, -min) over the ranks
            held = True if cmask is None else bool(np.array_equal(mine.points[cmask], glob.points[cmask]))
            if ebits is not None:
                held = held and mine.ext[eheld].tobytes() == glob.ext[eheld].tobytes()
            held = torch.tensor([1 if held else 0], dtype=torch.int32)
            dist.all_reduce(held, op=dist.ReduceOp.MIN)
            if rank == 0:
                rs, rp, re, rk = ref
                ca = [it["cost"] for it in summ["iterations"]]
                cb = [it["cost"] for it in rs["iterations"]]
                n = min(len(ca), len(cb))
                out[f"{kind}_{lst}"] = dict(
                    iters=(summ["num_iterations"], rs["num_iterations"]),
                    term=(summ["termination"], rs["termination"]),
                    max_rel_cost=float(max(abs(x - y) / abs(y) for x, y in zip(ca[:n], cb[:n]))),
                    cg_equal=[it["linear_solver_iterations"] for it in summ["iterations"]]
                    == [it["linear_solver_iterations"] for it in rs["iterations"]],
                    final=(summ["final_cost"], rs["final_cost"]),
                    dpts=float(np.abs(pts.numpy() - rp).max()),
                    dext=float(np.abs(ext.numpy() - re).max()),
                    ext_ranks_equal=bool(torch.equal(ext, ext_min)),
                    dintr=float((np.abs(kk.numpy() - rk) / np.maximum(1.0, np.abs(rk))).max()) if rk.size else 0.0,
                    intr_ranks_equal=bool(torch.equal(kk, kk_min)),
                    intr_moved=float(np.abs(rk - glob.intr).max()) if rk.size else 0.0,
                    num_parameters=(summ["num_parameters"], rs["num_parameters"]),
                    num_residuals=(summ["num_residuals"], rs["num_residuals"], 2 * glob.num_obs), prior_share=prior_share,
                    pt_prior_share=pt_prior_share, pt_effective=pt_eff,
                    intr_prior_share=intr_prior_share, intr_effective=intr_eff,
                    eval_schedule=sched, p2p=p2p,
                    assembly=(int(asm[0]), -int(asm[1]), rs["schur_assembly"]), const_held=bool(held.item()),
                    solver_used=(summ["linear_solver_type_used"], rs["linear_solver_type_used"]))
        for h in live:
            h.close()
    if rank == 0:
        print(json.dumps(out, indent=1))
        auto_want = names.get(a.expect_auto, None)
        bad = [k for k, v in out.items()
               if v["iters"][0] != v["iters"][1] or v["max_rel_cost"] > a.tol or v["dpts"] > 1e-6
               or (a.expect_cg_equal and not v["cg_equal"])
               or (auto_want is not None and k.endswith(f"_{pkg.DAB_LINEAR_SOLVER_AUTO}")
                   and v["solver_used"][0] != auto_want)
               or v["dext"] > 1e-6 or not v["ext_ranks_equal"]
               or v["dintr"] > 1e-6 or not v["intr_ranks_equal"]
               or (a.free_intrinsics and not v["intr_moved"] > 0.0)
               or (not k.startswith("rig") and v["eval_schedule"] != 2)  # BAL shards: the split fused pass
               or (a.expect_p2p and v["p2p"] != 1)
               or (a.expect_no_p2p and v["p2p"] != 0)
               or not v["const_held"]
               or (a.ext_priors and not (v["prior_share"] > 100 * a.tol and v["num_residuals"][1] > v["num_residuals"][2]))
               or (a.pt_priors and not (v["pt_prior_share"] > 100 * a.tol and 0 < v["pt_effective"][0] < v["pt_effective"][1]))
               or (a.intr_priors and not (v["intr_prior_share"] > 100 * a.tol and v["intr_effective"][0] > 0
                                          and v["num_residuals"][1] == v["num_residuals"][2] + 6 * v["intr_effective"][0]))
               or (a.const_points == "all" and v["solver_used"][0] == pkg.DAB_LINEAR_SOLVER_EXPLICIT_SCHUR
                   and v["assembly"] != (pkg.DAB_SCHUR_DIRECT,) * 3)
               or v["solver_used"][0] != v["solver_used"][1]]
        sys.stdout.write("DIST_CHECK " + ("FAIL " + ",".join(bad) if bad else "OK") + "\n")  # one write
        sys.stdout.flush()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
