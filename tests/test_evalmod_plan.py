"""The fused schedule of poly_eval_plan and the EvalMod plan, on the host alone.

The EvalMod bounds: float64 measures 8.0e-6 for evalmod_plan(4, 15, 2, 30) on
u = (I + eps) / 4, |I| <= 3, |eps| <= 2^-8 (4096 samples) against
sin(2 pi eps) / (2 pi) -- the interpolation error of the degree-15 cosine
through two double angles -- and 5.5e-10 for (16, 31, 3); the tests allow 2e-5
(2.5 x room for the sample) and 1e-8.
"""
from __future__ import annotations

import numpy as np
import pytest

from rns_ntt import evalmod_plan, poly_eval_plan, poly_eval_plan_fused
from rns_ntt.poly_eval import _build_plan

LOGP = 30
CASES = [(d, b) for d in (7, 15, 31) for b in ("monomial", "chebyshev")]


def _coeffs(d):
    return np.random.default_rng(900 + d).uniform(-1, 1, d + 1)


@pytest.mark.parametrize("d,basis", CASES)
def test_the_default_plan_is_unchanged(d, basis):
    """poly_eval_plan keeps its three parameters (tests/test_lincomb_exports.py
    pins them) and its plan: the shared builder with fused=False is the plan
    built without the switch, op for op, and emits no fma.  The reference tests
    (tests/test_poly_eval_ref.py, tests/test_gpu_poly_eval.py) pin its words."""
    c = _coeffs(d)
    old, new = poly_eval_plan(c, basis, LOGP), _build_plan(c, basis, LOGP, fused=False)
    assert old.ops == new.ops and old.levels == new.levels and old.result == new.result
    assert not any(op[0] == "fma" for op in old.ops)
    assert all(op[0] in ("drop", "mul", "add", "lincomb") for op in old.ops)
    fused = _build_plan(c, basis, LOGP, fused=True)
    pub = poly_eval_plan_fused(c, basis, LOGP)
    assert fused.ops == pub.ops and fused.levels == pub.levels and fused.result == pub.result


@pytest.mark.parametrize("d,basis", CASES)
def test_fused_plan_same_depth_and_leaves_same_values(d, basis):
    c = _coeffs(d)
    old, new = poly_eval_plan(c, basis, LOGP), poly_eval_plan_fused(c, basis, LOGP)
    assert new.depth == old.depth and new.n_leaves == old.n_leaves
    assert new.m == old.m and new.giants == old.giants
    # the leaves still come from the single rescaling lincomb, op for op
    assert [op for op in new.ops if op[0] == "lincomb" and op[5]] == [op for op in old.ops
                                                                      if op[0] == "lincomb" and op[5]]
    assert any(op[0] == "fma" for op in new.ops)
    if basis == "chebyshev":  # every recurrence step rides in its product
        assert not any(op[0] == "lincomb" and not op[5] for op in new.ops)
        n_powers = len(new.giants) + new.m - 2
        assert sum(op[0] == "fma" and op[4] == 2 for op in new.ops) == n_powers
    # fewer calls, never more
    assert len(new.ops) < len(old.ops)
    x = np.random.default_rng(3).uniform(-1, 1, 257)
    assert np.max(np.abs(new.evaluate_float(x) - old.evaluate_float(x))) < 1e-12


@pytest.mark.parametrize("d,basis", CASES)
def test_fma_operands_sit_where_the_call_needs_them(d, basis):
    plan = poly_eval_plan_fused(_coeffs(d), basis, LOGP)
    for op in plan.ops:
        if op[0] != "fma":
            continue
        _, dst, a, b, w, z, u, bias, fbias = op
        assert plan.levels[a] == plan.levels[b] == plan.levels[dst] - 1
        assert z is None or plan.levels[z] == plan.levels[dst]
        assert abs(w) < 2 ** 31 and abs(u) < 2 ** 31 and abs(bias) < 2 ** 62
        assert bias == int(np.rint(fbias * 2.0 ** LOGP))


def _inputs(K, seed=1, count=4096):
    rng = np.random.default_rng(seed)
    I = rng.integers(-(K - 1), K, count)
    eps = rng.uniform(-2.0 ** -8, 2.0 ** -8, count)
    return (I + eps) / K, eps


def test_evalmod_plan_4_15_2():
    plan = evalmod_plan(4, 15, 2, LOGP)
    assert plan.depth == 7 and plan.poly.depth == 5 and plan.double_angles == 2
    assert plan.poly.basis == "chebyshev" and not any(op[0] == "lincomb" and not op[5] for op in plan.poly.ops)
    a = (2 * np.pi) ** -0.25
    assert plan.constants == [int(np.rint(a ** 2 * 2.0 ** LOGP)), int(np.rint(a ** 4 * 2.0 ** LOGP))]
    u, eps = _inputs(4)
    err = float(np.max(np.abs(plan.evaluate_float(u) - np.sin(2 * np.pi * eps) / (2 * np.pi))))
    print(f"evalmod_plan(4, 15, 2): float64 error {err:.3e}")
    assert err < 2e-5


def test_evalmod_plan_16_31_3():
    plan = evalmod_plan(16, 31, 3, LOGP)
    assert plan.depth == 9
    u, eps = _inputs(16)
    err = float(np.max(np.abs(plan.evaluate_float(u) - np.sin(2 * np.pi * eps) / (2 * np.pi))))
    print(f"evalmod_plan(16, 31, 3): float64 error {err:.3e}")
    assert err < 1e-8


def test_evalmod_plan_refuses_nonsense():
    for args in ((0, 15, 2, 30), (4, 0, 2, 30), (4, 15, -1, 30), (4, 15, 2, 0), (4, 15, 2, 62)):
        with pytest.raises(ValueError):
            evalmod_plan(*args)
