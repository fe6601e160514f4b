"""The evaluation pass's blocks (V, g, U | g_c, the arc-ring cross blocks, the cost) block by
block, on every schedule one handle can take, at the smallest shapes that put each schedule on
an edge. Reference: tests/eval_blocks_ref.py (the CPU oracle's autodiff rows summed pairwise in
longdouble), pinned by tests/test_eval_blocks_ref.py. Every block is judged on its own scale.

Tolerances, from the project and not from the code under test: blocks 1e-9 of the block scale
(the bound test_gpu_parity.py states between two Jacobian evaluations, here per block), cost
1e-12 relative. Each case prints its worst error / (1e-9 * scale) per array.

Thresholds, from the code: kLdsCams = 1024 (dab_kernels.h: E, NI limit of the LDS point tables
and of the fused pass), kSmallTabs = 128 (dab_rows.h: E, NI limit of the pair-major pass and of
the staged cross pass), kChunk = 4096 entries per camera chunk, kPairChunk = 2560 records per
pair piece, kBalCW = kBalPW = 8 camera / point waves per fused work-group (dab_k_fused.hip),
SELL slice = 64 points. The fused pass's grid is the CU count: fused_wpc gives 8 waves per camera
up to NC = grid, 4 up to 2 grid, 2 up to 4 grid = the most that fuses; fused_wps gives 8 point
waves per slice up to grid slices, 4 up to 2 grid, 2 up to 4 grid, then 1, and also halves
while 12 E + 8 * 9 * 64 doubles exceed the 12 * kLdsCams table (E >= 641 -> 4). The sizes below
put those edges on a 256-CU grid (MI355X); on another CU count the cases still check their
blocks and their schedule (1024 free cameras fuse on >= 256 CUs), only the edge moves.

No rotation here has theta^2 in (DBL_EPSILON, 1e-10]: the autodiff reference loses digits there
(golden_util.py) and those have their own test. theta = 0 and |w| ~ 1e-9 are used.
"""
import numpy as np
import pytest

import eval_blocks_ref as eb
import robust_ref as rr

pytestmark = pytest.mark.gpu

TOL, TOL_COST = eb.TOL_BLOCK, eb.TOL_COST
KNOBS = ("DAB_CHUNK", "DAB_XCHUNK", "DAB_PAIR_EVAL", "DAB_EVAL_WPS", "DAB_EVAL_FUSED", "DAB_EVAL_SPLIT",
         "DAB_FUSED_TAB", "DAB_SETUP_HOST", "DAB_EVAL_SIDE", "DAB_BENCH_SAMPLE")


# ---- shapes -----------------------------------------------------------------------------------
def _bal(pkg, ncam, npt, opp, seed, **kw):
    return pkg.synth(kind=0, num_cameras=ncam, num_points=npt, obs_per_point=opp, seed=seed, **kw)


def _free_exact(prob, nfree, const=(0,)):
    """ext_const = `const` only; every other camera must be referenced, so NC is exactly nfree."""
    prob.ext_const[:] = 0
    prob.ext_const[list(const)] = 1
    assert len(eb.free_extrinsics(prob)) == nfree, len(eb.free_extrinsics(prob))
    return prob


def _reobserve(pkg, orc, prob, rng, noise=1.0):
    """Observe the projection at the current parameters, then pixel noise and perturbed points."""
    r, _ = orc.eval_residuals(pkg, prob)
    assert np.isfinite(r).all()
    prob.obs_xy += r
    prob.obs_xy += noise * rng.normal(size=prob.obs_xy.shape)
    prob.points += rng.normal(scale=1e-3, size=prob.points.shape)
    return prob


def _unit(rng):
    d = rng.normal(size=3)
    return d / np.linalg.norm(d)


def bal_one_free(pkg, orc):
    return _free_exact(_bal(pkg, 2, 70, 2, 101), 1)


def bal33_ragged(pkg, orc):
    """33 cameras / 200 points, tracks of 1..8, two one-observation points, camera 7 left with
    a single observation."""
    prob = rr._ragged(_bal(pkg, 33, 200, 8, 102), np.random.default_rng(102), 1, 8)
    of7 = np.flatnonzero(prob.obs_ext0 == 7)
    keep = np.ones(prob.num_obs, bool)
    keep[of7[1:]] = False
    prob = prob.subset(keep).copy()
    cnt = np.bincount(prob.obs_point, minlength=200)
    assert (prob.obs_ext0 == 7).sum() == 1 and (cnt == 1).sum() >= 2
    return prob


def bal_const_third(pkg, orc):
    """ext_const on a third of the cameras beyond the gauge: entries < observations."""
    prob = _bal(pkg, 33, 200, 4, 103)
    prob.ext_const[::3] = 1
    assert len(eb.free_extrinsics(prob)) == 22
    return prob


def bal_holes(pkg, orc):
    """Point 7 and camera 3 referenced by no observation: zero V, g rows, no ug row."""
    prob = _bal(pkg, 20, 150, 4, 104)
    sub = prob.subset((prob.obs_point != 7) & (prob.obs_ext0 != 3)).copy()
    assert 3 not in eb.free_extrinsics(sub)
    return sub


def bal_small_angles(pkg, orc):
    """Rotations on the small-angle branch: theta = 0 and |w| ~ 1e-9 (theta^2 <= DBL_EPSILON)."""
    prob = _bal(pkg, 24, 300, 4, 105)
    rng = np.random.default_rng(105)
    prob.ext[1, :3] = 0.0
    prob.ext[2, :3] = [1e-9, -2e-9, 3e-9]
    prob.ext[3, :3] = [0.0, 1.4e-8, 0.0]
    prob.ext[4, :3] = 1e-9 * _unit(rng)
    for e in (1, 2, 3, 4):
        prob.ext[e, 3:] = [rng.normal(scale=0.05), rng.normal(scale=0.05), 2.0]
    th2 = (prob.ext[:, :3] ** 2).sum(axis=1)
    assert not ((th2 > np.finfo(float).eps) & (th2 <= 1e-10)).any()
    return _reobserve(pkg, orc, prob, rng)


def _bal_big_rotations(pkg, orc, seed, above_pi):
    prob = _bal(pkg, 24, 300, 4, seed)
    rng = np.random.default_rng(seed)
    for e in range(prob.ext.shape[0]):
        th = rng.uniform(np.pi, np.pi + 0.05) if (above_pi and e % 4 == 1) else rng.uniform(2.5, np.pi - 1e-6)
        prob.ext[e, :3] = _unit(rng) * th
        prob.ext[e, 3:] = [rng.normal(scale=0.05), rng.normal(scale=0.05), 2.0]  # depth ~2: in front
    return _reobserve(pkg, orc, prob, rng)


def bal_rot_2p5_pi(pkg, orc):
    return _bal_big_rotations(pkg, orc, 106, False)


def bal_rot_above_pi(pkg, orc):
    prob = _bal_big_rotations(pkg, orc, 107, True)
    assert (np.linalg.norm(prob.ext[:, :3], axis=1) > np.pi).sum() >= 4
    return prob


def bal_1e8(pkg, orc):
    prob = _bal(pkg, 24, 300, 4, 108)
    prob.intr[:, :4] *= 1e8
    prob.obs_xy *= 1e8
    return prob


NOISE_FREE = dict(pixel_noise=0.0, point_noise=0.0, rot_noise=0.0, trans_noise=0.0)


def bal_noise_free(pkg, orc):
    return _bal(pkg, 24, 300, 4, 109, **NOISE_FREE)


def bal_chunked(pkg, orc):
    """3 cameras x 5000 points x 3: both free cameras hold 5000 > kChunk = 4096 entries, so
    nchunk = 4 != NC = 2: not fused, camera partials through k_seg_final."""
    return _free_exact(_bal(pkg, 3, 5000, 3, 110), 2)


def rig3x5_frozen(pkg, orc):
    prob = eb.rig_small(pkg)
    prob.freeze_camera = True
    return prob


def rig_1x2(pkg, orc):
    return pkg.synth(kind=1, num_arcs=1, num_rings=2, num_points=70, obs_per_point=2, seed=121)


def rig_2x1(pkg, orc):
    return pkg.synth(kind=1, num_arcs=2, num_rings=1, num_points=70, obs_per_point=2, seed=122)


def rig3x5(pkg, orc):
    prob = eb.rig_small(pkg)
    assert min(eb.obs_kinds(prob)) > 0, eb.obs_kinds(prob)
    return prob


def rig3x5_full(pkg, orc):
    """3 x 5, 200 points x 6 unthinned: ~80 records per pair, > 64 (the least DAB_XCHUNK takes)."""
    return pkg.synth(kind=1, num_arcs=3, num_rings=5, num_points=200, obs_per_point=6, seed=6)


def rig3x5_mixed(pkg, orc):
    """Arc 2's intrinsic duplicated and every other observation of it re-pointed at the copy
    (test_pair_eval_mixed_intrinsics' recipe, on the arc whose pairs are free): the pairs mix two
    intrinsics, so k_eval_pair reads per-record tables and arc 2's camera chunks are general."""
    q = eb.rig_small(pkg)
    ni = q.intr.shape[0]
    q.intr = np.ascontiguousarray(np.vstack([q.intr, q.intr[2:3]]))
    q.intr_nf = np.ascontiguousarray(np.append(q.intr_nf, q.intr_nf[2]).astype(np.int32))
    q.intr_nk = np.ascontiguousarray(np.append(q.intr_nk, q.intr_nk[2]).astype(np.int32))
    sel = np.flatnonzero(q.obs_intr == 2)[::2]
    q.obs_intr[sel] = ni
    assert ((q.obs_ext1 >= 0) & (q.obs_intr == ni)).sum() > 10
    return q


def rig3x5_one_intrinsic(pkg, orc):
    """One shared intrinsic for every camera."""
    q = eb.rig_small(pkg)
    q.obs_intr[:] = 0
    return q


def rig_2x2_long_pair(pkg, orc):
    """2 x 2, 3000 points x 4: the one free pair holds 3000 > kPairChunk = 2560 records (2 pieces)."""
    prob = pkg.synth(kind=1, num_arcs=2, num_rings=2, num_points=3000, obs_per_point=4, seed=123)
    assert eb.obs_kinds(prob)[1] == 3000
    return prob


def rig_e128(pkg, orc):
    prob = pkg.synth(kind=1, num_arcs=9, num_rings=120, num_points=2500, obs_per_point=2, seed=124)
    assert prob.ext.shape[0] == 128
    return prob


def rig_e129(pkg, orc):
    prob = pkg.synth(kind=1, num_arcs=9, num_rings=121, num_points=2500, obs_per_point=2, seed=125)
    assert prob.ext.shape[0] == 129
    return prob


def rig_rotations(pkg, orc):
    """3 x 5 with arcs near pi (one just above) and rings at theta = 0 and |w| ~ 1e-9. Points in a
    0.3 ball at the origin, ring translations (.., .., 2), arc translations (.., .., 3): depth
    >= 1.7 through a ring, >= 2.7 through an arc, >= 3 - |R1 X + t1| >= 0.6 composed."""
    prob = pkg.synth(kind=1, num_arcs=3, num_rings=5, num_points=200, obs_per_point=6, seed=126)
    rng = np.random.default_rng(126)
    prob.points[:] = [0.28 * _unit(rng) * rng.uniform() ** (1 / 3) for _ in range(200)]
    prob.ext[1, :3] = _unit(rng) * (np.pi - 1e-3)
    prob.ext[2, :3] = _unit(rng) * (np.pi + 0.02)
    prob.ext[3, :3] = 0.0
    prob.ext[4, :3] = 1e-9 * _unit(rng)
    prob.ext[5, :3] = _unit(rng) * 2.9
    prob.ext[6, :3] = _unit(rng) * 0.3
    for e in range(1, 7):
        prob.ext[e, 3:] = [rng.normal(scale=0.03), rng.normal(scale=0.03), 3.0 if e < 3 else 2.0]
    prob.ext[0] = 0.0
    prob.ext[0, 5] = 3.0
    return _reobserve(pkg, orc, prob, rng)


def _cams(nfree, seed, obs_per_cam=8):
    """nfree free cameras + the gauge, ~obs_per_cam observations each in tracks of 2."""
    def make(pkg, orc):
        ncam = nfree + 1
        for sd in range(seed, seed + 64000, 1000):  # the first seed of the series that references every camera
            prob = _bal(pkg, ncam, ncam * obs_per_cam // 2, 2, sd)
            if len(np.unique(prob.obs_ext0)) == ncam:
                return _free_exact(prob, nfree)
        raise AssertionError("no seed references every camera")
    return make


def bal_1024(pkg, orc):
    """E = NI = kLdsCams, no constant camera: NC = 1024 = 4 x 256, the most that fuses."""
    return _free_exact(_bal(pkg, 1024, 5120, 2, 131), 1024, const=())


def bal_1025(pkg, orc):
    return _free_exact(_bal(pkg, 1025, 5125, 2, 132), 1024)


def _slices(nslice, seed):
    def make(pkg, orc):
        prob = _bal(pkg, 40, 64 * (nslice - 1) + 1, 2, seed)
        assert -(-prob.points.shape[0] // 64) == nslice
        return prob
    return make


SHAPES = {
    "bal_one_free": bal_one_free, "bal33_ragged": bal33_ragged,
    "bal12_ragged": lambda pkg, orc: eb.bal_small(pkg),  # ~75 entries per camera
    "bal_63pt": lambda pkg, orc: _bal(pkg, 3, 63, 2, 111), "bal_64pt": lambda pkg, orc: _bal(pkg, 3, 64, 2, 112),
    "bal_65pt": lambda pkg, orc: _bal(pkg, 3, 65, 2, 113),
    "bal_nc256": _cams(256, 141), "bal_nc257": _cams(257, 142), "bal_nc512": _cams(512, 143),
    "bal_nc513": _cams(513, 144), "bal_e641": _cams(640, 145), "bal_1024": bal_1024, "bal_1025": bal_1025,
    "bal_257slices": _slices(257, 151), "bal_1025slices": _slices(1025, 152),
    "bal_chunked": bal_chunked, "bal_const_third": bal_const_third, "bal_holes": bal_holes,
    "bal_small_angles": bal_small_angles, "bal_rot_2p5_pi": bal_rot_2p5_pi, "bal_rot_above_pi": bal_rot_above_pi,
    "bal_1e8": bal_1e8, "bal_noise_free": bal_noise_free,
    "bal_gauge_only": lambda pkg, orc: _bal(pkg, 1, 7, 1, 114), "rig3x5_frozen": rig3x5_frozen,
    "rig_1x2": rig_1x2, "rig_2x1": rig_2x1, "rig3x5": rig3x5, "rig3x5_full": rig3x5_full,
    "rig3x5_mixed": rig3x5_mixed, "rig3x5_one_intrinsic": rig3x5_one_intrinsic,
    "rig_2x2_long_pair": rig_2x2_long_pair, "rig_e128": rig_e128, "rig_e129": rig_e129,
    "rig_rotations": rig_rotations,
}
# noise-free rows have rounding-sized residuals (|r| ~ 1e-13 px): g = J^T r is then rounding noise
# on both sides and sum m |r| is no scale for it. The project's residual bound is 1e-12 absolute
# below |r| = 1 (test_gpu_parity.py), so a residual may differ by 1e-12 and g by sum m 1e-12 =
# 1e-9 sum m 1e-3: at the block tolerance, that is a floor of 1e-3 px under |r| in the scale.
R_FLOOR = {"bal_noise_free": 1e-3}


@pytest.fixture(scope="module")
def shapes(pkg, orc):
    """name -> (problem, reference), each built once and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            prob = SHAPES[name](pkg, orc)
            cache[name] = (prob, eb.reference_blocks(pkg, orc, prob, R_FLOOR.get(name, 0.0)))
        return cache[name]
    return get


# ---- the one helper ---------------------------------------------------------------------------
def run_pass(pkg, monkeypatch, prob, env, fused, pair):
    """Blocks of one evaluation pass on a fresh handle under `env`; asserts the schedule that ran."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    s = pkg.Solver(0)
    try:
        s.set_problem(prob.copy())
        assert s.eval_fused() == fused, f"schedule {s.eval_fused()}, expected {fused} under {env}"
        assert (s.bench_pair_ms()[1] > 0) == pair, f"pair-major bytes {s.bench_pair_ms()[1]}, expected pair={pair}"
        s.bench_eval_pass(True, 1)
        s.sync()
        return s.bench_blocks()
    finally:
        s.close()


def check(got, ref, label, cost_abs=None):
    worst = eb.assert_blocks_close(got, ref, TOL)
    cref = float(ref["cost"])
    cerr = abs(got["cost"][0] - cref) / (cost_abs if cost_abs else cref)
    print(f"{label}: worst error / (1e-9 scale) " + " ".join(f"{k} {v:.2e}" for k, v in worst.items())
          + f"; cost error / 1e-12 {cerr / TOL_COST:.2e}")
    assert cerr <= TOL_COST, (got["cost"][0], cref)
    return worst


F0 = {"DAB_EVAL_FUSED": "0"}
WPS = ["-2", "0", "4", "8", "16", "-112", "-122", "-113"]

# (shape, route id, environment, expected dab_eval_schedule, pair-major pass expected)
CASES = []


def _add(shape, rid, env, fused, pair=False):
    CASES.append(pytest.param(shape, rid, env, fused, pair, id=f"{shape}-{rid}"))


# every shape the library evaluates in the fused launch (no composed observation, one chunk per
# camera, E, NI <= kLdsCams, NC <= 4 x grid): the single launch, the same kernel on prebuilt
# tables, and the two-kernel pass on its default point kernel
FUSED_SHAPES = ("bal_one_free", "bal33_ragged", "bal12_ragged", "bal_63pt", "bal_64pt", "bal_65pt", "bal_nc256",
                "bal_nc257", "bal_nc512", "bal_nc513", "bal_e641", "bal_1024", "bal_257slices", "bal_1025slices",
                "bal_const_third", "bal_holes", "bal_small_angles", "bal_rot_2p5_pi", "bal_rot_above_pi", "bal_1e8",
                "bal_noise_free", "rig_1x2", "rig_2x1")  # the two smallest rigs hold no composed observation
for _s in FUSED_SHAPES:
    _add(_s, "fused", {}, 1)
    _add(_s, "fused_tab", {"DAB_FUSED_TAB": "1"}, 1)
    _add(_s, "two_kernel", F0, 0)
# every point kernel of the two-kernel pass; the LDS and prefetch kernels (DAB_EVAL_WPS <= 0) hold
# E tables in LDS and are only reachable with E <= kLdsCams
for _s in ("bal33_ragged", "bal_65pt", "bal_nc257", "bal_const_third", "bal_small_angles", "bal_rot_above_pi",
           "bal_257slices"):
    for _w in WPS:
        _add(_s, f"two_kernel_wps{_w}", {**F0, "DAB_EVAL_WPS": _w}, 0)
for _w in ("-122", "16"):
    _add("bal_1025slices", f"two_kernel_wps{_w}", {**F0, "DAB_EVAL_WPS": _w}, 0)
    _add("bal_1024", f"two_kernel_wps{_w}", {**F0, "DAB_EVAL_WPS": _w}, 0)
# no free camera (the only camera is the gauge; freeze_camera): the point side alone, ug and ux empty
_add("bal_gauge_only", "no_free_camera", {}, 0)
_add("rig3x5_frozen", "no_free_camera", {}, 0)
_add("rig3x5_frozen", "no_free_camera_wps-112", {"DAB_EVAL_WPS": "-112"}, 0)
# E = 1025 > kLdsCams: schedule 0 unasked, k_eval_points<4 | 8 | 16> on global tables
_add("bal_1025", "global_tables", {}, 0)
_add("bal_1025", "global_tables_wps8", {"DAB_EVAL_WPS": "8"}, 0)
_add("bal_1025", "global_tables_wps16", {"DAB_EVAL_WPS": "16"}, 0)
# cameras cut into chunks (nchunk != NC): not fused, partials through k_seg_final
_add("bal_chunked", "seg_final", {}, 0)
for _w in WPS:
    _add("bal_chunked", f"seg_final_wps{_w}", {"DAB_EVAL_WPS": _w}, 0)
_add("bal12_ragged", "chunk64", {"DAB_CHUNK": "64"}, 0)  # the same route from a small shape: 2 chunks per camera
_add("bal33_ragged", "setup_host", {"DAB_SETUP_HOST": "1"}, 1)
_add("bal_chunked", "setup_host", {"DAB_SETUP_HOST": "1"}, 0)
_add("bal12_ragged", "setup_host_chunk64", {"DAB_SETUP_HOST": "1", "DAB_CHUNK": "64"}, 0)
# rigs with composed observations: the pair-major pass, or camera-major + k_eval_cross
for _s in ("rig3x5", "rig3x5_full", "rig3x5_mixed", "rig3x5_one_intrinsic", "rig_2x2_long_pair", "rig_e128",
           "rig_rotations"):
    _add(_s, "pair", {}, 0, True)
    _add(_s, "cross", {"DAB_PAIR_EVAL": "0"}, 0, False)
_add("rig_e129", "cross_global", {}, 0, False)  # E > kSmallTabs: no pair-major pass, k_eval_cross on global tables
_add("rig_e129", "cross_global_wps-112", {"DAB_EVAL_WPS": "-112"}, 0, False)
_add("rig3x5_full", "pair_xchunk", {"DAB_XCHUNK": "32"}, 0, True)   # the library takes max(64, DAB_XCHUNK): 2 pieces
_add("rig3x5_full", "cross_xchunk", {"DAB_XCHUNK": "32", "DAB_PAIR_EVAL": "0"}, 0, False)
_add("rig3x5_full", "pair_chunk64", {"DAB_CHUNK": "64"}, 0, True)
_add("rig3x5_full", "cross_chunk64", {"DAB_CHUNK": "64", "DAB_PAIR_EVAL": "0"}, 0, False)
_add("rig3x5", "setup_host", {"DAB_SETUP_HOST": "1"}, 0, True)
_add("rig3x5", "setup_host_cross", {"DAB_SETUP_HOST": "1", "DAB_PAIR_EVAL": "0"}, 0, False)
_add("rig_2x2_long_pair", "setup_host", {"DAB_SETUP_HOST": "1"}, 0, True)
_add("rig3x5_mixed", "setup_host", {"DAB_SETUP_HOST": "1"}, 0, True)
for _w in WPS:
    _add("rig3x5", f"pair_wps{_w}", {"DAB_EVAL_WPS": _w}, 0, True)
    _add("rig3x5", f"cross_wps{_w}", {"DAB_EVAL_WPS": _w, "DAB_PAIR_EVAL": "0"}, 0, False)
    _add("rig_rotations", f"pair_wps{_w}", {"DAB_EVAL_WPS": _w}, 0, True)


@pytest.mark.parametrize("shape,route,env,fused,pair", CASES)
def test_blocks_match_reference(pkg, orc, gpu, shapes, monkeypatch, shape, route, env, fused, pair):
    """One pass on the stated schedule against the reference, block by block."""
    prob, ref = shapes(shape)
    got = run_pass(pkg, monkeypatch, prob, env, fused, pair)
    cost_abs = None
    if shape == "bal_noise_free":
        # the cost is rounding-sized: absolute, at 1e-12 of the same shape's cost with 1 px noise
        noisy = _bal(pkg, 24, 300, 4, 109)
        cost_abs = orc.eval_residuals(pkg, noisy)[1]
        assert float(ref["cost"]) < 1e-12 * cost_abs
        raw = eb.block_ratios(got, eb.reference_blocks(pkg, orc, prob), TOL)  # printed only: no floor under |r|
        print(f"{shape}: without the residual floor g {raw['g'].max():.2e} gc {raw['gc'].max():.2e}")
    check(got, ref, f"{shape} [{route}]", cost_abs)
    if shape == "bal_holes":
        assert not got["V"][7].any() and not got["g"][7].any() and len(ref["free"]) == got["ug"].shape[0] == 18
    if shape == "bal_1e8":
        assert got["cost"][0] >= 1e20


@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_split_launch_is_bitwise_the_single_launch(pkg, orc, gpu, shapes, monkeypatch, shape):
    """DAB_EVAL_SPLIT=1 (schedule 2: the fused kernel as a camera-side and a point-side launch):
    close to the reference, and bitwise the blocks of the single launch."""
    prob, ref = shapes(shape)
    one = run_pass(pkg, monkeypatch, prob, {}, 1, False)
    two = run_pass(pkg, monkeypatch, prob, {"DAB_EVAL_SPLIT": "1"}, 2, False)
    cost_abs = orc.eval_residuals(pkg, _bal(pkg, 24, 300, 4, 109))[1] if shape == "bal_noise_free" else None
    check(two, ref, f"{shape} [split]", cost_abs)
    for k in one:
        np.testing.assert_array_equal(one[k], two[k], err_msg=k)


@pytest.mark.parametrize("shape,env,fused,pair", [
    pytest.param("bal33_ragged", {}, 1, False, id="fused"),
    pytest.param("bal33_ragged", {**F0, "DAB_EVAL_WPS": "-112"}, 0, False, id="prefetch"),
    pytest.param("rig3x5", {}, 0, True, id="rig")])
def test_state_across_passes(pkg, orc, gpu, shapes, monkeypatch, shape, env, fused, pair):
    """Passes 1, 2 and 3 give bitwise equal blocks and cost (the two alternating fixed-point
    cost sets and the zeroing of the next one); a pass after update_parameters matches the
    reference at the new x (no stale tables); back at the first x the first blocks return
    bitwise; set_points_constant on a third of the points changes nothing (raw quantities)."""
    prob, ref = shapes(shape)
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(7)
    moved = prob.copy()
    moved.points += rng.normal(scale=2e-3, size=moved.points.shape)
    free = eb.free_extrinsics(prob)
    moved.ext[free] += rng.normal(scale=1e-3, size=(len(free), 6))
    ref_moved = eb.reference_blocks(pkg, orc, moved)

    def same(a, b):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)

    s = pkg.Solver(0)
    try:
        s.set_problem(prob.copy())
        assert s.eval_fused() == fused and (s.bench_pair_ms()[1] > 0) == pair
        out = []
        for n in (1, 1, 1, 2):  # passes 1, 2, 3, then two in one batch
            s.bench_eval_pass(True, n)
            s.sync()
            out.append(s.bench_blocks())
        check(out[0], ref, f"{shape} [state: pass 1]")
        for b in out[1:]:
            same(out[0], b)
        s.update_parameters(moved.points, moved.ext)
        s.bench_eval_pass(True, 1)
        s.sync()
        check(s.bench_blocks(), ref_moved, f"{shape} [state: moved x]")
        s.update_parameters(prob.points, prob.ext)
        s.bench_eval_pass(True, 1)
        s.sync()
        same(out[0], s.bench_blocks())
        mask = np.zeros(prob.points.shape[0], np.uint8)
        mask[::3] = 1
        s.set_points_constant(mask)
        s.bench_eval_pass(True, 1)
        s.sync()
        same(out[0], s.bench_blocks())
    finally:
        s.close()
