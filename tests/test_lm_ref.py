"""Pins tests/lm_ref.py's lm() to the four loops it replaced (CPU only).

tests/golden/lm_ref_parent.json holds what robust_ref.lm, intr_ref.lm, ptconst_ref.lm and
prior_ref.lm returned at the last commit that had them (the file's header names it), on the cases
of oracle/gen_lm_ref_golden.py. On the recording machine the generator reproduces the file byte for
byte; here every case is held to the project's oracle-pin rule (tests/test_intr_ref.py's _same),
which is not bitwise because another machine's BLAS sums in another order: the same termination,
iteration count and success / valid flags, every iteration's cost and the final cost within 1e-9
relative, points and extrinsics within 1e-7, intrinsics within 1e-7 max(1, |value|), and the same
sizes."""
import json
import os

import numpy as np
import pytest

import gen_lm_ref_golden as gen
import lm_ref as lr
from golden_util import GOLDEN

GOLD = json.load(open(os.path.join(GOLDEN, "lm_ref_parent.json")))
CASES = GOLD["cases"]


@pytest.fixture(scope="module")
def made(pkg, orc):
    return dict(gen.cases(pkg, orc))


def test_file_holds_the_generators_cases(made):
    assert list(CASES) == list(made)
    assert len(GOLD["header"]["recorded_from"]) == 40 and GOLD["header"]["recorded_from"] == gen.PARENT
    assert GOLD["header"]["iteration_fields"] == list(gen.FLAGS + gen.FLOATS)
    for group in ("robust", "intr", "ptconst", "prior"):
        assert any(n.startswith(group + "/") for n in CASES)
    assert any(r["num_unsuccessful_steps"] > 0 for r in CASES.values())
    assert os.path.getsize(os.path.join(GOLDEN, "lm_ref_parent.json")) < 200 * 1000


@pytest.mark.parametrize("name", list(CASES))
def test_lm_reproduces_the_recorded_parent(pkg, orc, made, name):
    rec = CASES[name]
    prob, opts, kw = made[name]()
    s = lr.lm(pkg, orc, prob, opts, **kw)
    assert s["termination"] == rec["termination"], (s["message"], rec["message"])
    assert s["num_iterations"] == rec["num_iterations"]
    for k in ("num_parameters", "num_free_points", "num_free_ext", "num_residuals"):
        assert s[k] == rec[k], k
    assert [int(i["success"]) for i in s["iterations"]] == [r[0] for r in rec["iterations"]]
    assert [int(i["valid"]) for i in s["iterations"]] == [r[1] for r in rec["iterations"]]
    for x, r in zip(s["iterations"], rec["iterations"]):
        y = float.fromhex(r[2])
        assert abs(x["cost"] - y) <= 1e-9 * abs(y), (x, r)
    final = float.fromhex(rec["final_cost"])
    assert abs(s["final_cost"] - final) <= 1e-9 * final
    points = gen.unhex(rec["points"]).reshape(-1, 3)
    assert np.abs(prob.points[gen.first_points(prob)] - points).max() < 1e-7
    assert np.abs(prob.ext - gen.unhex(rec["ext"]).reshape(prob.ext.shape)).max() < 1e-7
    intr = gen.unhex(rec["intr"]).reshape(prob.intr.shape)
    assert (np.abs(prob.intr - intr) <= 1e-7 * np.maximum(1.0, np.abs(intr))).all()
