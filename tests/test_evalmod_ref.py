"""The CPU model of the fused plans (tests/evalmod_ref.py), without a GPU.

* FusedRunner's restatement of the four old ops gives PlanRunner.run's words.
* One fused call against plain decryption on a small ring: decryption is
  linear, so dec(w r + u z + bias) = w dec(r) + u dec(z) + bias X^0 mod q_t
  EXACTLY, with dec(r) taken from the multiply's own yardstick -- no tolerance.
* A fused plan gives the words of the unfused one wherever the two agree op
  for op up to the affine step (all of a Chebyshev plan): the affine step is
  exact, so the words are equal, not close.
* The decode errors of the fused evaluator and of EvalMod on the GPU tests'
  rings.  TOLERANCE: tools/evalmod_tolerance.py (profiles/evalmod_tolerance.txt),
  eight seeds, largest decode error at the nominal scale 2^30:

      degree  7 monomial  8.538e-04     degree  7 chebyshev 3.582e-03
      degree 15 monomial  2.238e-03     degree 15 chebyshev 1.608e-02
      evalmod (4, 15, 2)  1.199e-03     (against sin(2 pi eps) / (2 pi))

  The unfused composition measures the same figures to every printed digit.
  The tolerance is 4 x the maximum, the project's standing margin; most of
  every figure is the scale drift of q != 2^30 that the integer logp ignores.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
import rns_ntt
from evalmod_ref import FusedModel, affine_ref
from hybrid_rescale_ref import mul_relin_rescale_hybrid_ref
from poly_eval_ref import Model, plain_value

N, K, ALPHA, LOGP = 1024, 2, 2, 30
MEASURED = {(7, "monomial"): 8.538e-04, (7, "chebyshev"): 3.582e-03,
            (15, "monomial"): 2.238e-03, (15, "chebyshev"): 1.608e-02}
EVALMOD_MEASURED = 1.199e-03


@pytest.fixture(scope="module")
def ring7():
    return orc.generate_primes(LOGP, 7, N), orc.generate_primes(31, K, N)


@pytest.mark.parametrize("d,basis", [(7, "chebyshev"), (15, "monomial")])
def test_restated_ops_give_plan_runners_words(ring7, d, basis):
    old, new = Model(*ring7, N, ALPHA, LOGP, seed=5), FusedModel(*ring7, N, ALPHA, LOGP, seed=5)
    x = old.rng.uniform(-1, 1, N // 2)
    coeffs = old.rng.uniform(-1, 1, d + 1)
    ct = old.encrypt(x)
    plan = rns_ntt.poly_eval_plan(coeffs, basis, LOGP)
    a, b = old.runner.run(plan, ct), new.runner.run(plan, ct)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("w,u,bias", [(2, -1, 0), (2, None, -(1 << 30)), (-3, 5, (1 << 61) - 1), (0, 1, -1)])
def test_one_fused_call_against_plain_decryption(w, u, bias):
    n, L = 64, 4
    q, p = orc.generate_primes(LOGP, L, n), orc.generate_primes(31, K, n)
    m = FusedModel(q, p, n, ALPHA, LOGP, seed=11)
    x, y, zv = (m.rng.uniform(-1, 1, n // 2) for _ in range(3))
    cx, cy = m.encrypt(x), m.encrypt(y)
    z = tuple(np.ascontiguousarray(c[:L - 1]) for c in m.encrypt(zv)) if u is not None else None
    got = m.runner.fma(cx, cy, w, z, u or 0, bias)
    assert got[0].shape == (L - 1, n)
    Bc, Be, ka, kb = m.runner.level(L)
    Bl = m.runner.level(L - 1)[0]
    sk = m.sk[:L - 1]

    def dec(ct):
        return orc.add(Bl, orc.mul(Bl, ct[1], sk), ct[0])

    r = mul_relin_rescale_hybrid_ref(Bc, Be, *cx, *cy, ka, kb, ALPHA)
    want = np.zeros_like(got[0])
    dr, dz = dec(r), (dec(z) if z is not None else None)
    for t, qt in enumerate(q[:L - 1]):
        acc = dr[t].astype(object) * w
        if dz is not None:
            acc = acc + dz[t].astype(object) * u
        acc[0] += bias
        want[t] = (acc % int(qt)).astype(np.uint64)
    assert np.array_equal(dec(got), want)
    # and the words themselves are affine_ref of the yardstick's
    a0, a1 = affine_ref(q[:L - 1], r[0], r[1], w, z, u or 0, bias)
    assert np.array_equal(got[0], a0) and np.array_equal(got[1], a1)


def test_fused_chebyshev_plan_gives_the_unfused_words(ring7):
    m = FusedModel(*ring7, N, ALPHA, LOGP, seed=6)
    x = m.rng.uniform(-1, 1, N // 2)
    coeffs = m.rng.uniform(-1, 1, 8)
    ct = m.encrypt(x)
    a = m.runner.run(rns_ntt.poly_eval_plan(coeffs, "chebyshev", LOGP), ct)
    b = m.runner.run(rns_ntt.poly_eval_plan_fused(coeffs, "chebyshev", LOGP), ct)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("d,basis", sorted(MEASURED))
def test_fused_evaluator_decode_error(ring7, d, basis):
    m = FusedModel(*ring7, N, ALPHA, LOGP, seed=2000 + d)
    x = m.rng.uniform(-1, 1, N // 2)
    coeffs = m.rng.uniform(-1, 1, d + 1)
    plan = rns_ntt.poly_eval_plan_fused(coeffs, basis, LOGP)
    out = m.runner.run(plan, m.encrypt(x))
    assert out[0].shape == (7 - plan.depth, N)
    err = float(np.max(np.abs(m.decode(out) - plain_value(coeffs, basis, x))))
    print(f"fused degree {d} {basis}: decode error {err:.3e} (tolerance {4 * MEASURED[(d, basis)]:.3e})")
    assert err < 4 * MEASURED[(d, basis)]


def test_evalmod_decode_error():
    q, p = orc.generate_primes(LOGP, 9, N), orc.generate_primes(31, K, N)
    m = FusedModel(q, p, N, ALPHA, LOGP, seed=3000)
    I = m.rng.integers(-3, 4, N // 2)
    eps = m.rng.uniform(-2.0 ** -8, 2.0 ** -8, N // 2)
    plan = rns_ntt.evalmod_plan(4, 15, 2, LOGP)
    out = m.runner.run_evalmod(plan, m.encrypt((I + eps) / 4))
    assert out[0].shape == (9 - plan.depth, N) == (2, N)
    err = float(np.max(np.abs(m.decode(out) - np.sin(2 * np.pi * eps) / (2 * np.pi))))
    print(f"evalmod (4, 15, 2): decode error {err:.3e} (tolerance {4 * EVALMOD_MEASURED:.3e})")
    assert err < 4 * EVALMOD_MEASURED
