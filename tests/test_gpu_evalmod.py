"""The fused polynomial evaluator and EvalMod on the GPU
(CkksEngine.evaluate_polynomial_hybrid_fused, CkksEngine.eval_mod_hybrid):
word for word the CPU execution of the same plans (tests/evalmod_ref.py), the
decode against numpy, and the launch counts -- every Chebyshev recurrence step
and every double angle is ONE mul_ciphertexts_hybrid_rescale_affine, so a
fused evaluation launches k_lincomb once (the leaves).

Rings: N = 2^10, ciphertext primes of 30 bits (7 for the evaluator, as
tests/test_gpu_poly_eval.py; 9 for EvalMod), K = 2 special primes of 31 bits,
alpha = 2, B = 2 ciphertexts, scale 2^30, ONE full-level relinearisation key.

TOLERANCE: tools/evalmod_tolerance.py (profiles/evalmod_tolerance.txt), eight
seeds of the CPU model on these rings, largest decode error at the nominal
scale 2^30:

    degree  7 monomial  8.538e-04     degree  7 chebyshev 3.582e-03
    degree 15 monomial  2.238e-03     degree 15 chebyshev 1.608e-02
    evalmod (4, 15, 2)  1.199e-03     (inputs (I + eps) / 4, |I| <= 3, |eps| <= 2^-8,
                                       against sin(2 pi eps) / (2 pi))

The unfused composition measures the same figures.  They include the scale drift
of q != 2^30 that the engine's integer logp ignores (most of them).  The
tolerance is 4 x the maximum, the project's standing margin for the
seed-to-seed spread of the noise.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from evalmod_ref import FusedModel
from poly_eval_ref import plain_value

pytestmark = pytest.mark.gpu

N, K, ALPHA, LOGP, B = 1024, 2, 2, 30, 2
MEASURED = {(7, "monomial"): 8.538e-04, (7, "chebyshev"): 3.582e-03,
            (15, "monomial"): 2.238e-03, (15, "chebyshev"): 1.608e-02}
EVALMOD_MEASURED = 1.199e-03
EVALMOD = (4, 15, 2)


class Setup:
    """The CPU model (keys, B encrypted inputs) and its device twin."""

    def __init__(self, rn, L, seed, inputs):
        self.L = L
        self.q, self.p = orc.generate_primes(LOGP, L, N), orc.generate_primes(31, K, N)
        self.model = m = FusedModel(self.q, self.p, N, ALPHA, LOGP, seed=seed)
        self.x = [inputs(m.rng) for _ in range(B)]
        self.cts = [m.encrypt(v) for v in self.x]
        self.ext = rn.RnsBasis(self.q + self.p, N)
        self.basis = self.ext.drop_last(K)
        self.key = rn.RnsHybridKey.from_channels(m.key_a, m.key_b, self.ext, ALPHA, n_special=K)
        c0 = rn.RnsPoly.from_channels(np.stack([c[0] for c in self.cts]), self.basis)
        c1 = rn.RnsPoly.from_channels(np.stack([c[1] for c in self.cts]), self.basis)
        self.ct = rn.Ciphertext(c0, c1, LOGP, self.basis.total_bits())


@pytest.fixture(scope="module")
def eval_setup(gpu):
    return Setup(gpu, 7, 4242, lambda rng: rng.uniform(-1, 1, N // 2))


def _evalmod_inputs(rng):
    I = rng.integers(-(EVALMOD[0] - 1), EVALMOD[0], N // 2)
    return (I + rng.uniform(-2.0 ** -8, 2.0 ** -8, N // 2)) / EVALMOD[0]


@pytest.fixture(scope="module")
def mod_setup(gpu):
    return Setup(gpu, 9, 4343, _evalmod_inputs)


def _profiled(basis, run, names):
    basis.profile_enable(True)
    try:
        out = run()
        return out, {k: basis.profile_read(k)[0] for k in names}
    finally:
        basis.profile_enable(False)


@pytest.mark.parametrize("d,basis", sorted(MEASURED))
def test_fused_evaluator(gpu, eval_setup, d, basis):
    rn = gpu
    from rns_ntt.engine import CkksEngine

    s = eval_setup
    coeffs = np.random.default_rng(77 + d).uniform(-1, 1, d + 1)
    plan = rn.poly_eval_plan_fused(coeffs, basis, LOGP)
    n_fma = sum(op[0] == "fma" for op in plan.ops)
    n_mul = sum(op[0] == "mul" for op in plan.ops)
    got, n = _profiled(s.basis, lambda: CkksEngine.evaluate_polynomial_hybrid_fused(s.ct, coeffs, s.key, basis=basis),
                       ("lincomb", "moddown_rescale_affine", "moddown_rescale"))
    assert n == {"lincomb": 1, "moddown_rescale_affine": 2 * n_fma, "moddown_rescale": 2 * n_mul}, n
    lv = s.L - plan.depth
    assert got.c0.basis.channel_count() == lv and got.c0.n_polys == B
    assert got.logp == LOGP and got.logq == s.ct.logq - LOGP * plan.depth
    assert not got.c0.is_ntt_domain() and not got.c1.is_ntt_domain()
    w0, w1 = got.c0.channels_batch(), got.c1.channels_batch()
    tol = 4 * MEASURED[(d, basis)]
    for b in sorted({0, B - 1}):
        r0, r1 = s.model.runner.run(plan, s.cts[b])
        assert np.array_equal(w0[b], r0), f"c0 of ciphertext {b} differs from the CPU execution of the fused plan"
        assert np.array_equal(w1[b], r1), f"c1 of ciphertext {b} differs from the CPU execution of the fused plan"
        err = float(np.max(np.abs(s.model.decode((w0[b], w1[b])) - plain_value(coeffs, basis, s.x[b]))))
        print(f"fused degree {d} {basis}, ciphertext {b}: decode error {err:.3e} (tolerance {tol:.3e})")
        assert err < tol


def test_eval_mod(gpu, mod_setup):
    rn = gpu
    from rns_ntt.engine import CkksEngine

    s = mod_setup
    plan = rn.evalmod_plan(*EVALMOD, LOGP)
    assert plan.depth == 7
    n_fma = sum(op[0] == "fma" for op in plan.poly.ops) + plan.double_angles
    n_mul = sum(op[0] == "mul" for op in plan.poly.ops)
    got, n = _profiled(s.basis, lambda: CkksEngine.eval_mod_hybrid(s.ct, plan, s.key),
                       ("lincomb", "moddown_rescale_affine", "moddown_rescale"))
    assert n == {"lincomb": 1, "moddown_rescale_affine": 2 * n_fma, "moddown_rescale": 2 * n_mul}, n
    assert got.c0.basis.channel_count() == 2 and got.c0.n_polys == B and got.c0.basis is got.c1.basis
    assert got.logp == LOGP and got.logq == s.ct.logq - LOGP * plan.depth
    w0, w1 = got.c0.channels_batch(), got.c1.channels_batch()
    tol = 4 * EVALMOD_MEASURED
    for b in sorted({0, B - 1}):
        r0, r1 = s.model.runner.run_evalmod(plan, s.cts[b])
        assert np.array_equal(w0[b], r0), f"c0 of ciphertext {b} differs from the CPU model"
        assert np.array_equal(w1[b], r1), f"c1 of ciphertext {b} differs from the CPU model"
        t = s.x[b] * EVALMOD[0]  # I + eps with |eps| <= 2^-8
        eps = t - np.rint(t)
        err = float(np.max(np.abs(s.model.decode((w0[b], w1[b])) - np.sin(2 * np.pi * eps) / (2 * np.pi))))
        print(f"evalmod {EVALMOD}, ciphertext {b}: decode error {err:.3e} (tolerance {tol:.3e})")
        assert err < tol


def test_eval_mod_refuses_what_it_cannot_run(gpu, mod_setup):
    rn = gpu
    from rns_ntt.engine import CkksEngine

    s = mod_setup
    plan = rn.evalmod_plan(*EVALMOD, LOGP)
    with pytest.raises(ValueError, match="levels"):  # 7 levels: 8 limbs are fine, 7 are not
        low = rn.Ciphertext(s.ct.c0.mod_drop_last(2), s.ct.c1.mod_drop_last(2), LOGP, s.ct.logq - 2 * LOGP)
        CkksEngine.eval_mod_hybrid(low, plan, s.key)
    with pytest.raises(ValueError, match="bits"):  # the consumed primes must have logp bits
        CkksEngine.eval_mod_hybrid(rn.Ciphertext(s.ct.c0, s.ct.c1, 29, s.ct.logq), rn.evalmod_plan(*EVALMOD, 29), s.key)
    with pytest.raises(ValueError, match="logp"):  # a plan made for another scale
        CkksEngine.eval_mod_hybrid(s.ct, rn.evalmod_plan(*EVALMOD, 29), s.key)
