"""CPU tests of the evaluation-pass block reference (tests/eval_blocks_ref.py) and of its
comparator. The GPU matrix (test_gpu_eval_blocks.py) trusts both only because these pin them:
the reference against itself under reordering and against a dense J^T J, and the comparator
against the mutations a reduction kernel produces when it goes wrong, at the GPU tolerance."""
import numpy as np
import pytest

import eval_blocks_ref as eb

LD = np.longdouble
TOL = eb.TOL_BLOCK


@pytest.fixture(scope="module")
def cases(pkg, orc):
    out = {}
    for name, make in (("bal", eb.bal_small), ("rig", eb.rig_small)):
        prob = make(pkg)
        r, J = orc.eval_jacobians(pkg, prob)
        out[name] = (prob, r, J, eb.blocks_from_rows(prob, r, J))
    return out


def as_got(ref):
    """The reference rounded to the float64 arrays dab_bench_get_blocks would return."""
    return {k: np.array(ref[k], np.float64) for k in ("V", "g", "ug", "ux")}


def test_longdouble_is_extended():
    """The reference's rounding bound (1e-17 of the block scale) needs a 64-bit mantissa."""
    assert np.finfo(LD).eps <= 2.0 ** -63


def test_shapes_are_ragged(cases):
    prob, _, _, ref = cases["bal"]
    assert prob.ext.shape[0] == 12 and prob.points.shape[0] == 200
    assert ref["V_count"].min() == 1 and ref["V_count"].max() == 8 and (ref["V_count"] == 2).any()
    assert len(ref["free"]) == 11 and ref["U_count"].min() >= 50 and ref["ux"].shape == (0, 36)
    prob, _, _, ref = cases["rig"]
    assert prob.ext.shape[0] == 7 and min(eb.obs_kinds(prob)) > 0, eb.obs_kinds(prob)
    assert list(ref["free"]) == [2, 3, 4, 5, 6] and [tuple(p) for p in ref["pairs"]] == [(2, 3), (2, 4), (2, 5), (2, 6)]


def test_segsum_is_exact_on_integers():
    rng = np.random.default_rng(1)
    key = rng.integers(0, 37, size=5000)
    key[key == 11] = 12  # an empty group
    t = rng.integers(-2 ** 40, 2 ** 40, size=(5000, 3))
    s = eb.segsum(key, 37, t)
    for j in range(37):
        assert (s[j] == t[key == j].sum(axis=0)).all()


@pytest.mark.parametrize("name", ["bal", "rig"])
def test_observation_order_does_not_matter(cases, name):
    prob, r, J, ref = cases[name]
    perm = np.random.default_rng(3).permutation(prob.num_obs)
    sh = eb.blocks_from_rows(prob.subset(perm), r[perm], J[perm])
    q = eb.block_ratios(sh, ref, 1e-16)
    print({k: float(v.max()) if len(v) else 0.0 for k, v in q.items()})
    assert all((v <= 1.0).all() for v in q.values())
    assert abs(sh["cost"] - ref["cost"]) <= 1e-17 * ref["cost"]
    for k in ("free", "pairs", "V_count", "U_count", "ux_count"):
        np.testing.assert_array_equal(sh[k], ref[k])
    for k in ("V_scale", "g_scale", "U_scale", "gc_scale", "ux_scale"):
        np.testing.assert_allclose(sh[k], ref[k], rtol=1e-13)


@pytest.mark.parametrize("name", ["bal", "rig"])
def test_point_labels_do_not_matter(cases, name):
    prob, r, J, ref = cases[name]
    npts = prob.points.shape[0]
    new_of = np.random.default_rng(4).permutation(npts)  # old label -> new label
    rel = prob.copy()
    rel.obs_point = new_of[prob.obs_point].astype(np.int32)
    rel.points = np.empty_like(prob.points)
    rel.points[new_of] = prob.points
    rb = eb.blocks_from_rows(rel, r, J)
    for k in ("V", "g", "V_scale", "g_scale", "V_count"):
        np.testing.assert_array_equal(rb[k][new_of], ref[k])  # same terms in the same order: bitwise
    for k in ("ug", "ux"):
        np.testing.assert_array_equal(rb[k], ref[k])


@pytest.mark.parametrize("name", ["bal", "rig"])
def test_matches_dense_normal_matrix(cases, name):
    """An independent formation: the dense [2 N][n] Jacobian over (referenced points, free
    extrinsics) in longdouble, H = A^T A and A^T r, the diagonal and the arc-ring blocks cut out.
    The dense products sum in observation order, not pairwise: 1e-15 of the block scale."""
    prob, r, J, ref = cases[name]
    free = ref["free"]
    npts, nc, N = prob.points.shape[0], len(free), prob.num_obs
    col = np.full(prob.ext.shape[0] + 1, -1, np.int64)
    col[free] = np.arange(nc)
    A = np.zeros((2 * N, 3 * npts + 6 * nc), LD)
    rows = 2 * np.arange(N)
    for k in range(3):
        A[rows, 3 * prob.obs_point + k] = J[:, 0, k]
        A[rows + 1, 3 * prob.obs_point + k] = J[:, 1, k]
    for ext, k0 in ((prob.obs_ext0, 3), (prob.obs_ext1, 9)):
        c = col[ext]
        ok = np.flatnonzero(c >= 0)
        for k in range(6):
            A[rows[ok], 3 * npts + 6 * c[ok] + k] = J[ok, 0, k0 + k]
            A[rows[ok] + 1, 3 * npts + 6 * c[ok] + k] = J[ok, 1, k0 + k]
    H = A.T @ A
    b = A.T @ np.asarray(r, LD).ravel()
    V = np.stack([H[3 * p:3 * p + 3, 3 * p:3 * p + 3][eb.IU3] for p in range(npts)])
    o = 3 * npts
    U = np.stack([H[o + 6 * c:o + 6 * c + 6, o + 6 * c:o + 6 * c + 6][eb.IU6] for c in range(nc)])
    gc = b[o:].reshape(nc, 6)
    ux = [H[o + 6 * col[a]:o + 6 * col[a] + 6, o + 6 * col[b_]:o + 6 * col[b_] + 6].reshape(36)
          for a, b_ in ref["pairs"]]
    dense = dict(V=V, g=b[:o].reshape(npts, 3), ug=np.concatenate([U, gc], axis=1),
                 ux=np.stack(ux) if ux else np.zeros((0, 36), LD))
    q = eb.block_ratios(dense, ref, 1e-15)
    print({k: float(v.max()) if len(v) else 0.0 for k, v in q.items()})
    assert all((v <= 1.0).all() for v in q.values())
    # and no other arc-ring block of H is non-zero: the pair list is complete
    mask = np.zeros((nc, nc), bool)
    for a, b_ in ref["pairs"]:
        mask[col[a], col[b_]] = mask[col[b_], col[a]] = True
    Hc = np.abs(H[o:, o:]).reshape(nc, 6, nc, 6).max(axis=(1, 3))
    assert (Hc[~mask & ~np.eye(nc, dtype=bool)] == 0).all()
    assert abs(ref["cost"] - LD(0.5) * (np.asarray(r, LD) ** 2).sum()) <= 1e-17 * ref["cost"]


def test_unmutated_copy_passes(cases):
    for name in ("bal", "rig"):
        ref = cases[name][3]
        worst = eb.assert_blocks_close(as_got(ref), ref, TOL)
        assert max(worst.values()) <= 1e-6  # float64 rounding of the entries: 1e-16 / 1e-9


def _obs_of_ext(prob, e):
    return np.flatnonzero((prob.obs_ext0 == e) | (prob.obs_ext1 == e))


def m_drop_from_large_camera(prob, r, J, ref):
    """The last observation of a camera with >= 50 left out of its U | g_c."""
    c = int(np.argmax(ref["U_count"]))
    assert ref["U_count"][c] >= 50
    k = _obs_of_ext(prob, ref["free"][c])[-1:]
    a, b, _ = eb.obs_terms(r[k], J[k], slice(3, 9))
    got = as_got(ref)
    got["ug"][c] = np.array(ref["ug"][c] - np.concatenate([a[0], b[0]]), np.float64)
    return got, "U", c


def m_drop_from_two_observation_point(prob, r, J, ref):
    p = int(np.flatnonzero(ref["V_count"] == 2)[0])
    k = np.flatnonzero(prob.obs_point == p)[-1:]
    a, b, _ = eb.obs_terms(r[k], J[k], slice(0, 3))
    got = as_got(ref)
    got["V"][p] = np.array(ref["V"][p] - a[0], np.float64)
    got["g"][p] = np.array(ref["g"][p] - b[0], np.float64)
    return got, "V", p


def m_padding_term_added(prob, r, J, ref):
    """A padding slot that repeats the track's last observation, added to one point block."""
    p = int(np.argmax(ref["V_count"]))
    k = np.flatnonzero(prob.obs_point == p)[-1:]
    a, b, _ = eb.obs_terms(r[k], J[k], slice(0, 3))
    got = as_got(ref)
    got["V"][p] = np.array(ref["V"][p] + a[0], np.float64)
    got["g"][p] = np.array(ref["g"][p] + b[0], np.float64)
    return got, "V", p


def m_row_scaled(prob, r, J, ref):
    """One Jacobian row of one camera (the row holding its largest entry) times 1 + 1e-7."""
    c = int(np.argmin(ref["U_count"]))
    ks = _obs_of_ext(prob, ref["free"][c])
    rowmax = np.abs(J[ks][:, :, 3:9]).max(axis=2)
    i, row = np.unravel_index(np.argmax(rowmax), rowmax.shape)
    J2 = J.copy()
    J2[ks[i], row, 3:9] *= 1.0 + 1e-7
    return as_got(eb.blocks_from_rows(prob, r, J2)), "U", c


def m_cross_swapped(prob, r, J, ref):
    got = as_got(ref)
    got["ux"][[1, 2]] = got["ux"][[2, 1]]
    return got, "ux", 1


def m_cross_transposed(prob, r, J, ref):
    got = as_got(ref)
    got["ux"][2] = got["ux"][2].reshape(6, 6).T.reshape(36)
    return got, "ux", 2


def m_packed_order(prob, r, J, ref):
    """One U block packed column by column of the upper triangle instead of row by row."""
    got = as_got(ref)
    M = np.zeros((6, 6))
    M[eb.IU6] = got["ug"][3, :21]
    got["ug"][3, :21] = M.T[np.tril_indices(6)]
    return got, "U", 3


def m_gc_negated(prob, r, J, ref):
    got = as_got(ref)
    got["ug"][2, 21:] *= -1.0
    return got, "gc", 2


# (mutation, problem, does the whole-array criterion it replaces let it through)
MUTATIONS = [
    (m_drop_from_large_camera, "bal", False),
    (m_drop_from_two_observation_point, "bal", False),
    (m_padding_term_added, "bal", False),
    (m_row_scaled, "bal", False),
    (m_cross_swapped, "rig", True),
    (m_cross_transposed, "rig", True),
    (m_packed_order, "bal", False),
    (m_gc_negated, "rig", False),
    (m_drop_from_large_camera, "rig", False),
    (m_row_scaled, "rig", False),
]


@pytest.mark.parametrize("mutate,name,old_passes", MUTATIONS, ids=[f"{m.__name__[2:]}-{n}" for m, n, _ in MUTATIONS])
def test_comparator_catches(cases, mutate, name, old_passes):
    """Each mutation of a copy of the reference fails assert_blocks_close at the GPU tolerance,
    in the array and block that was mutated; old_passes records whether the criterion this
    comparator replaces (1e-9 of the array's largest entry, cross blocks by their sum) lets the
    same mutation through."""
    prob, r, J, ref = cases[name]
    got, arr, blk = mutate(prob, r, J, ref)
    q = eb.block_ratios(got, ref, TOL)
    print(f"{mutate.__name__} on {name}: {arr}[{blk}] ratio {q[arr][blk]:.3g}, "
          f"{int(ref[arr + '_count'][blk])} observations; old criterion passes: {eb.old_criterion_passes(got, ref)}")
    assert q[arr][blk] > 1.0
    with pytest.raises(AssertionError, match=rf"\b{arr}: "):
        eb.assert_blocks_close(got, ref, TOL)
    assert eb.old_criterion_passes(got, ref) == old_passes


def test_old_criterion_misses_a_drop_beside_large_blocks(cases):
    """What the per-block scale adds, on the drops: next to blocks 1e10 times larger (here one
    camera's rows times 1e5: its pixel scale, as a mixed-resolution set has), a dropped observation of a 50-observation camera and of a 2-observation point
    both pass 1e-9 of the array's largest entry by orders of magnitude; per block they are off
    by 1e7 tolerances."""
    prob, r, J, _ = cases["bal"]
    cam = 5
    s = np.where(prob.obs_ext0 == cam, 1e5, 1.0)
    r2, J2 = r * s[:, None], J * s[:, None, None]  # the rows of that problem, exactly
    ref = eb.blocks_from_rows(prob, r2, J2)
    only_small = np.flatnonzero(np.bincount(prob.obs_point, weights=(s > 1), minlength=len(ref["V_count"])) == 0)
    p = int(only_small[ref["V_count"][only_small] == 2][0])
    c = int(np.flatnonzero(ref["free"] != cam)[0])
    assert ref["U_count"][c] >= 50
    for arr, blk, k, cols in (("U", c, _obs_of_ext(prob, ref["free"][c])[-1:], slice(3, 9)),
                              ("V", p, np.flatnonzero(prob.obs_point == p)[-1:], slice(0, 3))):
        a, b, _ = eb.obs_terms(r2[k], J2[k], cols)
        got = as_got(ref)
        if arr == "U":
            got["ug"][blk] = np.array(ref["ug"][blk] - np.concatenate([a[0], b[0]]), np.float64)
        else:
            got["V"][blk] = np.array(ref["V"][blk] - a[0], np.float64)
            got["g"][blk] = np.array(ref["g"][blk] - b[0], np.float64)
        q = eb.block_ratios(got, ref, TOL)
        print(f"{arr}[{blk}]: per-block ratio {q[arr][blk]:.3g}; old criterion passes: "
              f"{eb.old_criterion_passes(got, ref)}")
        assert eb.old_criterion_passes(got, ref)
        with pytest.raises(AssertionError, match=rf"\b{arr}: "):
            eb.assert_blocks_close(got, ref, TOL)
