"""TEST INFRASTRUCTURE ONLY: the cases and masks of the constant-point tests (a plain module).

The reference's solve() keeps `//problem.SetParameterBlockConstant(parameter_block[0]); //freeze
point3d` commented out (sfm.cc:59); the library's switch for it is dab_set_points_constant. Ceres
removes constant blocks from the program it minimises, so the reference is lm_ref.lm / lm_ref.covariance
with `const`: constant points get no columns in lm_ref.Layout; their observations keep their rows
and their camera and intrinsic columns. Here are the cases and masks the CPU and GPU tests share.
"""
import numpy as np

import robust_ref as rr


# ---- the cases of the constant-point tests ------------------------------------------------------
def case_b(pkg):
    """BAL-shaped: 24 cameras, 200 points x 6 (rejected steps)."""
    return pkg.synth(kind=0, num_cameras=24, num_points=200, obs_per_point=6, seed=8, rot_noise=0.2,
                     trans_noise=0.4, point_noise=0.02)


def case_b_low(pkg):
    """B's base at lower noise (no rejected steps): the PCG comparisons."""
    return pkg.synth(kind=0, num_cameras=24, num_points=200, obs_per_point=6, seed=8, rot_noise=0.1,
                     trans_noise=0.2, point_noise=0.01)


def case_r(pkg):
    """Rig: 4 arcs x 6 rings, 200 points x 6."""
    return pkg.synth(kind=1, num_arcs=4, num_rings=6, num_points=200, obs_per_point=6, seed=7, rot_noise=0.1,
                     trans_noise=0.2, point_noise=0.01)


def case_r2(pkg):
    """The rig at higher noise (rejected steps): all-constant masks only. With mixed masks the
    reference differs from itself by up to 3e-2 between two observation orders at rot >= 0.15."""
    return pkg.synth(kind=1, num_arcs=4, num_rings=6, num_points=200, obs_per_point=6, seed=8, rot_noise=0.15,
                     trans_noise=0.3, point_noise=0.02)


def case_b_ragged(pkg):
    """B's base with tracks of 2-6 observations (padding slots, slices with mixed lanes). The
    generator's seed is 5 (cov_ref.bal40_ragged's), chosen by the reference's own spread between
    two observation orders with every third point constant, 25 iterations: 1.7e-11 of the cost
    (seeds 1, 2, 3: 2.9e-11, 1.3e-11, 2.4e-12). With seed 8 one rejected candidate has cost 2.2e35
    (a point next to a camera's plane) and the reference differs from itself by 1.3e-7 there: a
    parity test on that listing would pin nothing."""
    return rr._ragged(case_b(pkg), np.random.default_rng(5), 2, 6)


def every_third(prob):
    m = np.zeros(prob.points.shape[0], bool)
    m[::3] = True
    return m


def all_points(prob):
    return np.ones(prob.points.shape[0], bool)


def all_but_first5(prob):
    m = np.ones(prob.points.shape[0], bool)
    m[:5] = False
    return m


MASKS = {"third": every_third, "all": all_points, "allbut5": all_but_first5}
CASES = {"B": case_b, "R": case_r, "R2": case_r2, "Bragged": case_b_ragged}
RAGGED = ("Bragged", "third", None, 25)
CAUCHY2 = (rr.CAUCHY, 2.0)
# (case, mask, loss, max_num_iterations): the trajectories of the issue's table
TRAJECTORIES = [
    ("B", "third", None, 25), ("B", "all", None, 25), ("B", "allbut5", None, 25),
    ("B", "third", CAUCHY2, 15), ("B", "all", CAUCHY2, 15),
    ("R", "third", None, 25), ("R", "all", None, 25), ("R", "third", CAUCHY2, 15),
    ("R2", "all", None, 25),
]


def traj_id(t):
    return f"{t[0]}-{t[1]}" + ("-cauchy" if t[2] else "")
