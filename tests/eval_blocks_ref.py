"""TEST INFRASTRUCTURE ONLY: the host reference of the evaluation pass's blocks (a plain module).

What dab_bench_get_blocks returns after one pass, formed from the CPU oracle's rows
(orc.eval_jacobians: autodiff, Ceres-equivalent) in np.longdouble:
  V  [num_points][6]  J_p^T J_p upper-packed, caller's point order (zero rows for unreferenced points)
  g  [num_points][3]  J_p^T r
  ug [free][27]       U = J_c^T J_c upper-packed (21) | g_c = J_c^T r (6) per free extrinsic
                      (referenced and not constant), ascending extrinsic index
  ux [pairs][36]      J_c0^T J_c1 row-major (rows: the arc ext0's six columns, columns: the ring
                      ext1's) per (arc, ring) pair with at least one composed observation whose
                      two cameras are free, ordered by col(ext0) * NC + col(ext1) ascending, col =
                      rank among the free extrinsics (dab_problem.hip, "arc∘ring cross blocks";
                      orientation read from k_eval_cross: acc[6 a + b] += j0[a] * j1[b])
  cost                0.5 sum r^2
Every block's terms are summed pairwise (a balanced tree per block), so the reference's own
rounding is <= (1 + log2 n) 2^-64 sum|terms|: 1.6e-18 of the block scale at n = 5000 terms.

Block scales, returned alongside and used by the comparator instead of the block's own largest
entry (g cancels to almost nothing near a minimum). With m_k the largest |J| entry of
observation k over the columns the block uses (both rows):
  V, U: sum_k m_k^2      g, g_c: sum_k m_k max|r_k|      cross: sum_k m_k^(c0) m_k^(c1)
These bound the sum of the absolute values of the terms of every entry of the block, which is
what a summation in another order can differ by (times the unit round-off and log n).

assert_blocks_close judges every block on its own scale and names the one that fails.
"""
import numpy as np

import robust_ref as rr

TOL_BLOCK = 1e-9   # per block, on the block's scale: test_gpu_parity.py's bound between two Jacobian evaluations
TOL_COST = 1e-12   # relative

LD = np.longdouble
IU3 = np.triu_indices(3)
IU6 = np.triu_indices(6)
ARRAYS = ("V", "g", "U", "gc", "ux")


def segsum(key, n, terms):
    """out[j] = sum of terms[key == j] in longdouble, each group by a balanced pairwise tree.
    key [m] ints in [0, n), terms [m][K]. Groups are padded with zeros (exact) to a power of two
    and halved; groups are bucketed by padded length, so ragged sizes cost no more than 2x."""
    key = np.asarray(key, np.int64)
    terms = np.asarray(terms, LD)
    K = int(np.prod(terms.shape[1:], dtype=np.int64))
    terms = terms.reshape(len(key), K)
    out = np.zeros((n, K), LD)
    if len(key) == 0:
        return out
    order = np.argsort(key, kind="stable")
    k, t = key[order], terms[order]
    cnt = np.bincount(key, minlength=n)
    start = np.cumsum(cnt) - cnt
    rank = np.arange(len(k)) - start[k]
    size = np.ones(n, np.int64)
    big = cnt > 1
    size[big] = 2 ** np.ceil(np.log2(cnt[big])).astype(np.int64)
    size[cnt > size] *= 2  # guard the float log2 at exact powers
    ksize = size[k]
    for L in np.unique(size[cnt > 0]):
        grp = np.flatnonzero((size == L) & (cnt > 0))
        slot = np.full(n, -1, np.int64)
        slot[grp] = np.arange(len(grp))
        sel = ksize == L
        buf = np.zeros((len(grp), int(L), K), LD)
        buf[slot[k[sel]], rank[sel]] = t[sel]
        w = int(L)
        while w > 1:
            w //= 2
            buf = buf[:, :w] + buf[:, w:2 * w]
        out[grp] = buf[:, 0]
    return out


def free_extrinsics(prob):
    """Ascending indices of the extrinsics that are referenced and not constant."""
    ne = prob.ext.shape[0]
    ref = np.zeros(ne, bool)
    ref[prob.obs_ext0] = True
    ref[prob.obs_ext1[prob.obs_ext1 >= 0]] = True
    const = np.zeros(ne, bool) if prob.ext_const is None else prob.ext_const.astype(bool)
    if prob.freeze_camera:
        const[:] = True
    return np.flatnonzero(ref & ~const)


def obs_terms(r, J, cols):
    """Per-observation contribution to a diagonal block over J's columns `cols`: (JtJ upper-packed
    [N][n (n + 1) / 2], Jtr [N][n], m [N]) in longdouble, m in float64."""
    Jc = np.asarray(J[:, :, cols], LD)
    rl = np.asarray(r, LD)
    n = Jc.shape[2]
    iu = np.triu_indices(n)
    JtJ = Jc[:, 0, iu[0]] * Jc[:, 0, iu[1]] + Jc[:, 1, iu[0]] * Jc[:, 1, iu[1]]
    Jtr = Jc[:, 0, :] * rl[:, 0:1] + Jc[:, 1, :] * rl[:, 1:2]
    m = np.abs(J[:, :, cols]).reshape(len(J), -1).max(axis=1) if len(J) else np.zeros(0)
    return JtJ, Jtr, m


def cross_terms(J):
    """Per-observation J_c0^T J_c1, [N][36] row-major (rows ext0's columns), longdouble."""
    J0, J1 = np.asarray(J[:, :, 3:9], LD), np.asarray(J[:, :, 9:15], LD)
    X = J0[:, 0, :, None] * J1[:, 0, None, :] + J0[:, 1, :, None] * J1[:, 1, None, :]
    return X.reshape(len(J), 36)


def blocks_from_rows(prob, r, J, r_floor=0.0):
    """The blocks, their scales and their observation counts from rows r [N][2], J [N][2][15]
    (columns X | w0 t0 | w1 t1). r_floor: the g and g_c scales take max(max|r_k|, r_floor) per
    observation (0 everywhere but on noise-free inputs, whose residuals are rounding-sized: see
    test_gpu_eval_blocks.py). Returns a dict:
      V, g, ug, ux, cost (longdouble);  U = ug[:, :21], gc = ug[:, 21:]
      V_scale, g_scale [num_points]; U_scale, gc_scale [free]; ux_scale [pairs]
      V_count [num_points], U_count [free], ux_count [pairs]: observations (entries) per block
      free [free]: extrinsic index per ug row; pairs [pairs][2]: (ext0, ext1) per ux row."""
    npts, ne = prob.points.shape[0], prob.ext.shape[0]
    N = prob.num_obs
    rmax = np.maximum(np.abs(r).max(axis=1), r_floor) if N else np.zeros(0)
    # points
    VtV, Vtr, mp = obs_terms(r, J, slice(0, 3))
    V = segsum(prob.obs_point, npts, VtV)
    g = segsum(prob.obs_point, npts, Vtr)
    V_scale = np.bincount(prob.obs_point, weights=mp * mp, minlength=npts)
    g_scale = np.bincount(prob.obs_point, weights=mp * rmax, minlength=npts)
    V_count = np.bincount(prob.obs_point, minlength=npts)
    # cameras: the entries of both slots
    free = free_extrinsics(prob)
    nc = len(free)
    col = np.full(ne + 1, -1, np.int64)  # [-1] stays -1 (ext1 < 0)
    col[free] = np.arange(nc)
    keys, tU, tg, ms, rs = [], [], [], [], []
    for ext, cols in ((prob.obs_ext0, slice(3, 9)), (prob.obs_ext1, slice(9, 15))):
        c = col[ext]
        sel = np.flatnonzero(c >= 0)
        a, b, m = obs_terms(r[sel], J[sel], cols)
        keys.append(c[sel]); tU.append(a); tg.append(b); ms.append(m); rs.append(rmax[sel])
    key = np.concatenate(keys)
    m, rm = np.concatenate(ms), np.concatenate(rs)
    ug = np.concatenate([segsum(key, nc, np.concatenate(tU)), segsum(key, nc, np.concatenate(tg))], axis=1)
    U_scale = np.bincount(key, weights=m * m, minlength=nc)
    gc_scale = np.bincount(key, weights=m * rm, minlength=nc)
    U_count = np.bincount(key, minlength=nc)
    # arc-ring cross blocks
    c0, c1 = col[prob.obs_ext0], col[prob.obs_ext1]
    sel = np.flatnonzero((prob.obs_ext1 >= 0) & (c0 >= 0) & (c1 >= 0))
    pk = c0[sel] * max(nc, 1) + c1[sel]
    upk, inv = np.unique(pk, return_inverse=True)  # ascending key: the library's order
    ux = segsum(inv, len(upk), cross_terms(J[sel]))
    m0 = np.abs(J[sel][:, :, 3:9]).reshape(len(sel), -1).max(axis=1) if len(sel) else np.zeros(0)
    m1 = np.abs(J[sel][:, :, 9:15]).reshape(len(sel), -1).max(axis=1) if len(sel) else np.zeros(0)
    ux_scale = np.bincount(inv, weights=m0 * m1, minlength=len(upk))
    ux_count = np.bincount(inv, minlength=len(upk))
    pairs = np.stack([free[upk // max(nc, 1)], free[upk % max(nc, 1)]], axis=1) if len(upk) else np.zeros((0, 2), np.int64)
    rl = np.asarray(r, LD).ravel()
    cost = LD(0.5) * segsum(np.zeros(len(rl), np.int64), 1, (rl * rl)[:, None])[0, 0]
    return dict(V=V, g=g, ug=ug, U=ug[:, :21], gc=ug[:, 21:], ux=ux, cost=cost,
                V_scale=V_scale, g_scale=g_scale, U_scale=U_scale, gc_scale=gc_scale, ux_scale=ux_scale,
                V_count=V_count, g_count=V_count, U_count=U_count, gc_count=U_count, ux_count=ux_count,
                free=free, pairs=pairs)


def reference_blocks(pkg, orc, prob, r_floor=0.0):
    """blocks_from_rows of the CPU oracle's residuals and autodiff Jacobians at prob's parameters."""
    r, J = orc.eval_jacobians(pkg, prob)
    return blocks_from_rows(prob, r, J, r_floor)


def split_got(got):
    """A dab_bench_get_blocks dict (V, g, ug, ux) or a reference dict as the five compared arrays."""
    ug = np.asarray(got["ug"])
    return dict(V=np.asarray(got["V"]), g=np.asarray(got["g"]), U=ug[:, :21], gc=ug[:, 21:],
                ux=np.asarray(got["ux"]))


def _name(ref, arr, i):
    if arr in ("V", "g"):
        return f"point {i}"
    if arr in ("U", "gc"):
        return f"extrinsic {int(ref['free'][i])} (free rank {i})"
    return f"pair (arc ext {int(ref['pairs'][i][0])}, ring ext {int(ref['pairs'][i][1])}) (cross block {i})"


def block_ratios(got, ref, tol):
    """Per array, max|got - ref| / (tol * scale) of every block ([blocks] float64). A block of
    scale 0 (no observation) must be exactly zero: ratio 0, or inf."""
    a = split_got(got)
    out = {}
    for arr in ARRAYS:
        x, y = a[arr], np.asarray(ref[arr])
        assert x.shape == y.shape, f"{arr}: shape {x.shape}, reference {y.shape}"
        if x.shape[0] == 0:
            out[arr] = np.zeros(0)
            continue
        bad = ~np.isfinite(np.asarray(x, np.float64)).all(axis=1)
        err = np.abs(np.asarray(x, LD) - np.asarray(y, LD)).max(axis=1).astype(np.float64)
        scale = np.asarray(ref[arr + "_scale"], np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(scale > 0, err / (tol * scale), np.where(err == 0, 0.0, np.inf))
        ratio[bad] = np.inf
        out[arr] = ratio
    return out


def assert_blocks_close(got, ref, tol):
    """Every block of got (dab_bench_get_blocks' dict) within tol x its own scale of ref
    (blocks_from_rows' dict): max|got - ref| <= tol * scale per block. A failure names the
    array, the block (point, extrinsic or pair), its observation count and the ratio. Returns
    the worst ratio err / (tol * scale) per array."""
    ratios = block_ratios(got, ref, tol)
    worst, fails = {}, []
    for arr in ARRAYS:
        q = ratios[arr]
        worst[arr] = float(q.max()) if len(q) else 0.0
        nbad = int((~(q <= 1.0)).sum())
        if nbad:
            i = int(np.argmax(np.where(np.isnan(q), np.inf, q)))
            fails.append(f"{arr}: {nbad} of {len(q)} blocks off; worst {_name(ref, arr, i)}, "
                         f"{int(ref[arr + '_count'][i])} observations, "
                         f"error / (tol * scale) = {q[i]:.3g} (tol {tol:g}, scale {ref[arr + '_scale'][i]:.3g})")
    assert not fails, "; ".join(fails)
    return worst


def old_criterion_passes(got, ref, tol=1e-9):
    """The whole-array criterion this module replaces (test_bench_blocks_match_jacobian_kernel
    before it): every array within tol of its own largest entry, the cross blocks by the sum of
    all their entries. True when it does NOT flag `got`."""
    a = split_got(got)
    for arr in ("V", "g", "U", "gc"):
        y = np.asarray(ref[arr], np.float64)
        if y.size and np.abs(np.asarray(a[arr], np.float64) - y).max() > tol * np.abs(y).max():
            return False
    x, y = np.asarray(a["ux"], np.float64), np.asarray(ref["ux"], np.float64)
    return bool(abs(x.sum() - y.sum()) <= tol * np.abs(x).sum())


# ---- the problems the CPU and GPU tests share ---------------------------------------------
def bal_small(pkg):
    """12 cameras, 200 points, tracks of 1..8 (robust_ref's thinning recipe)."""
    base = pkg.synth(kind=0, num_cameras=12, num_points=200, obs_per_point=8, seed=5)
    return rr._ragged(base, np.random.default_rng(5), 1, 8)


def rig_small(pkg):
    """3 arcs x 5 rings, 200 points, tracks of 1..6. The synthesiser writes arc 0's cameras as
    single-extrinsic observations (of the ring, or of arc 0 itself), so its constant arc 0 never
    sits in a composed one; arc 1 is held constant too, which gives all three kinds: single,
    composed with both cameras free (arc 2) and composed with a constant arc (arc 1)."""
    base = pkg.synth(kind=1, num_arcs=3, num_rings=5, num_points=200, obs_per_point=6, seed=6)
    base.ext_const[1] = 1
    return rr._ragged(base, np.random.default_rng(6), 1, 6)


def obs_kinds(prob):
    """(single, composed with both cameras free, composed with a constant camera) counts."""
    const = np.zeros(prob.ext.shape[0], bool) if prob.ext_const is None else prob.ext_const.astype(bool)
    comp = prob.obs_ext1 >= 0
    cf = comp & ~const[prob.obs_ext0] & ~const[np.maximum(prob.obs_ext1, 0)]
    return int((~comp).sum()), int(cf.sum()), int((comp & ~cf).sum())
