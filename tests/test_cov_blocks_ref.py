"""The reference of dab_covariance_blocks (tests/cov_blocks_ref.py), pinned on the CPU:
  1. its slices of cov_ref.sigma_inv agree with the same slices of cov_ref.sigma_pinv within the
     project's bound (64 kappa 2^-53 max |Sigma|) on every case tests/test_gpu_cov_blocks.py uses;
  2. the three Schur formulas of the library's route, restated in numpy from the point factors, the
     records and C = S^-1 (schur_blocks), reproduce the slices within the bound: signs, scales and
     record sums are checked before any kernel runs;
  3. the comparator fails on a transposed block, a pe block without its minus sign, a missing s_c,
     one dropped record of a point, and (a, b) answered in (b, a)'s point order;
  4. the ABI table declares dab_covariance_blocks."""
import ctypes as C

import numpy as np
import pytest

import cov_blocks_ref as cbr
import cov_blocks_cases as cases
import cov_ref as cr

_cache = {}


def ref_of(pkg, orc, name):
    if name not in _cache:
        _cache[name] = cases.reference(pkg, orc, name)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_slices_agree_with_the_pseudo_inverse(pkg, orc, name):
    ref = ref_of(pkg, orc, name)
    L = ref["layout"]
    P = cr.sigma_pinv(ref["A"])
    if hasattr(L, "expand"):
        P = L.expand(P)
    pp, pe, pz = cbr.pair_lists(ref["prob"], 3)
    want, exact = cbr.slices(ref, pp, pe, pz)
    got, _ = cbr.slices(dict(ref, Sigma=P), pp, pe, pz)
    frac = cbr.compare(got, want, exact, ref["bound"])
    print(f"{name}: sigma_inv vs sigma_pinv slices, {frac:.3g} of the bound {ref['bound']:.3e}")
    assert sum(np.isfinite(want[k]).all(axis=(1, 2)).sum() for k in want) > 20


@pytest.mark.parametrize("name", ["rig3x5", "bal40", "rig6x20-mixed-g7", "rig6x20-mixed-masks", "extsub-trans-all",
                                  "ptconst-third", "soft-gauge", "cauchy"])
def test_schur_formulas_reproduce_the_slices(pkg, orc, name):
    ref = ref_of(pkg, orc, name)
    parts = cbr.schur_parts(ref)
    pp, pe, pz = cbr.pair_lists(ref["prob"], 4)
    want, exact = cbr.slices(ref, pp, pe, pz)
    got, _ = cbr.schur_blocks(ref, parts, pp, pe, pz)
    frac = cbr.compare(got, want, exact, ref["bound"])
    print(f"{name}: Schur formulas vs slices, {frac:.3g} of the bound {ref['bound']:.3e}")


@pytest.mark.parametrize("wrong", ["transpose", "sign", "scale", "record", "order"])
def test_comparator_catches(pkg, orc, wrong):
    ref = ref_of(pkg, orc, "rig3x5")  # well conditioned: the bound is far under every block's size
    parts = cbr.schur_parts(ref)
    pp, pe, pz = cbr.pair_lists(ref["prob"], 4)
    want, exact = cbr.slices(ref, pp, pe, pz)
    got, _ = cbr.schur_blocks(ref, parts, pp, pe, pz, wrong=wrong)
    with pytest.raises(AssertionError):
        cbr.compare(got, want, exact, ref["bound"])


def test_comparator_catches_misplaced_nan_and_negative_zero(pkg, orc):
    ref = ref_of(pkg, orc, "ptconst-third")
    pp, pe, pz = cbr.pair_lists(ref["prob"], 4)
    want, exact = cbr.slices(ref, pp, pe, pz)
    assert exact["pp"].any() and exact["pe"].any()
    cbr.compare(want, want, exact, ref["bound"])
    bad = {k: v.copy() for k, v in want.items()}
    bad["pp"][exact["pp"]] = -0.0
    with pytest.raises(AssertionError):
        cbr.compare(bad, want, exact, ref["bound"])
    bad = {k: v.copy() for k, v in want.items()}
    bad["pe"][0, 0, 0] = np.nan
    with pytest.raises(AssertionError):
        cbr.compare(bad, want, exact, ref["bound"])


def test_abi_declares_the_call(pkg):
    import importlib
    abi = importlib.import_module(pkg.__name__ + "._abi")
    res, args = abi.SIGNATURES["dab_covariance_blocks"]
    assert res is C.c_int and len(args) == 9
    req = abi.DabCovBlocksRequest()
    assert [f[0] for f in req._fields_] == ["num_pp", "pp", "num_pe", "pe", "num_pz", "pz"]
    assert hasattr(pkg.Solver, "covariance_blocks")
