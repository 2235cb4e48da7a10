"""rns_ntt.poly_eval_plan (a pure host function) and its CPU execution
(tests/poly_eval_ref.py), without a GPU: the plan's depth, the plan on plain
floats against numpy, and the decode error of the CPU model on the GPU test's
ring (N = 2^10, 7 x 30-bit primes, K = 2, alpha = 2, scale 2^30).

TOLERANCE: tools/poly_eval_tolerance.py, eight seeds, largest decode error
against numpy.polyval / chebval of the plain inputs (inputs and coefficients
uniform in (-1, 1); the error includes the scale drift of q_last != 2^30 that
the integer logp ignores):

    degree  7 monomial  8.538e-04     degree  7 chebyshev 3.582e-03
    degree 15 monomial  2.238e-03     degree 15 chebyshev 1.608e-02

The tolerance is 4 x that maximum, the project's standing margin.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
import rns_ntt
from poly_eval_ref import Model, plain_value

N, L, K, ALPHA, LOGP = 1024, 7, 2, 2, 30
MEASURED = {(7, "monomial"): 8.538e-04, (7, "chebyshev"): 3.582e-03,
            (15, "monomial"): 2.238e-03, (15, "chebyshev"): 1.608e-02}
TOLERANCE = {k: 4 * v for k, v in MEASURED.items()}
# the levels the schedule consumes, worked out by hand from its definition
# (babies to ceil(log2(m - 1)), the leaves one below, one per giant split)
DEPTH = {1: 1, 2: 2, 3: 2, 5: 4, 7: 4, 15: 5, 31: 6}


@pytest.mark.parametrize("basis", ["monomial", "chebyshev"])
@pytest.mark.parametrize("d", sorted(DEPTH))
def test_plan_depth_and_shape(d, basis):
    rng = np.random.default_rng(d)
    plan = rns_ntt.poly_eval_plan(rng.uniform(-1, 1, d + 1), basis, LOGP)
    bound = int(np.ceil(np.log2(d + 1))) + 1
    assert plan.depth == DEPTH[d] <= bound
    assert plan.m == max(2, 2 ** int(np.ceil(np.log2(d + 1) / 2)))
    assert plan.giants == [g for g in (plan.m << k for k in range(8)) if g <= d]
    # all leaves from one rescaling lincomb (none of these has more than 16)
    resc = [op for op in plan.ops if op[0] == "lincomb" and op[5]]
    assert len(resc) == 1 and len(resc[0][2]) == plan.m - 1 and 1 <= plan.n_leaves <= 16
    # every operand is used at the level the plan states, results one below
    for op in plan.ops:
        if op[0] in ("mul", "add"):
            assert plan.levels[op[2]] == plan.levels[op[3]]
            assert plan.levels[op[1]] == plan.levels[op[2]] + (op[0] == "mul")
        elif op[0] == "lincomb":
            assert len({plan.levels[s] for s in op[2]}) == 1
            assert all(plan.levels[x] == plan.levels[op[2][0]] + int(op[5]) for x in op[1])
            assert len(op[1]) <= 16 and len(op[2]) <= 16


@pytest.mark.parametrize("basis", ["monomial", "chebyshev"])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 7, 8, 15, 16, 31, 40])
def test_plan_on_floats_matches_numpy(d, basis):
    rng = np.random.default_rng(100 + d)
    coeffs = rng.uniform(-1, 1, d + 1)
    x = rng.uniform(-1, 1, 64)
    plan = rns_ntt.poly_eval_plan(coeffs, basis, LOGP)
    assert np.max(np.abs(plan.evaluate_float(x) - plain_value(coeffs, basis, x))) < 1e-12


def test_plan_weights_and_sparse_polynomials():
    # x^8 alone: m = 4, giants 4 and 8; the remainder of the split is zero, so no add
    plan = rns_ntt.poly_eval_plan([0] * 8 + [1.0], "monomial", LOGP)
    assert not [op for op in plan.ops if op[0] == "add"]
    x = np.linspace(-1, 1, 9)
    assert np.allclose(plan.evaluate_float(x), x ** 8, atol=1e-12)
    # the leaf weights are rint(c_k 2^p), the bias rint(c_0 2^2p); a constant leaf is bias-only
    plan = rns_ntt.poly_eval_plan([0.5, -0.25, 0.0, 0.0, 0.125], "monomial", LOGP)
    (op,) = [op for op in plan.ops if op[0] == "lincomb"]
    # (the quotient 0.125 is the first leaf, the remainder 0.5 - 0.25 x the second)
    assert op[3] == [[0, 0, 0], [-(1 << 28), 0, 0]] and op[4] == [1 << 57, 1 << 59]
    with pytest.raises(ValueError):
        rns_ntt.poly_eval_plan([1.0], "monomial", LOGP)
    with pytest.raises(ValueError):
        rns_ntt.poly_eval_plan([1.0, 2.0], "legendre", LOGP)


@pytest.fixture(scope="module")
def ring():
    return orc.generate_primes(LOGP, L, N), orc.generate_primes(31, K, N)


@pytest.mark.parametrize("d,basis", sorted(MEASURED))
def test_cpu_model_decode_error(ring, d, basis):
    model = Model(*ring, N, ALPHA, LOGP, seed=1000 + d)
    x = model.rng.uniform(-1, 1, N // 2)
    coeffs = model.rng.uniform(-1, 1, d + 1)
    plan = rns_ntt.poly_eval_plan(coeffs, basis, LOGP)
    out = model.runner.run(plan, model.encrypt(x))
    assert out[0].shape == (L - plan.depth, N)
    err = float(np.max(np.abs(model.decode(out) - plain_value(coeffs, basis, x))))
    print(f"degree {d} {basis}: decode error {err:.3e} (tolerance {TOLERANCE[(d, basis)]:.3e})")
    assert err < TOLERANCE[(d, basis)]
