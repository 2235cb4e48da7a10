"""CkksEngine.evaluate_polynomial_hybrid on the GPU: word for word the CPU
execution of the same plan (tests/poly_eval_ref.py on rns_ntt.poly_eval_plan),
its decode against numpy, and the launch count of k_lincomb.

Ring: N = 2^10, 7 ciphertext primes of 30 bits, K = 2 special primes of 31
bits, alpha = 2, B = 2 ciphertexts, scale 2^30; ONE full-level relinearisation
key, whose level views the multiplies pick by themselves.

TOLERANCE: tools/poly_eval_tolerance.py, eight seeds of the CPU model on this
ring, largest decode error at the nominal scale 2^30 against numpy.polyval /
chebval of the plain inputs (inputs and coefficients uniform in (-1, 1)):

    degree  7 monomial  8.538e-04     degree  7 chebyshev 3.582e-03
    degree 15 monomial  2.238e-03     degree 15 chebyshev 1.608e-02

The figures include the scale drift of q_last != 2^30, which the engine's
integer logp ignores (it is most of them: against a float model that carries
the true scale the same runs differ by 1e-5 .. 7e-4).  The tolerance is 4 x the
maximum, the project's standing margin for the seed-to-seed spread of the noise.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from poly_eval_ref import Model, plain_value

pytestmark = pytest.mark.gpu

N, L, K, ALPHA, LOGP, B = 1024, 7, 2, 2, 30, 2
MEASURED = {(7, "monomial"): 8.538e-04, (7, "chebyshev"): 3.582e-03,
            (15, "monomial"): 2.238e-03, (15, "chebyshev"): 1.608e-02}


class Setup:
    """The CPU model (keys, two encrypted inputs) and its device twin, shared
    by every case and left unchanged."""

    def __init__(self, rn):
        self.q, self.p = orc.generate_primes(LOGP, L, N), orc.generate_primes(31, K, N)
        self.model = m = Model(self.q, self.p, N, ALPHA, LOGP, seed=4242)
        self.x = [m.rng.uniform(-1, 1, N // 2) for _ in range(B)]
        self.cts = [m.encrypt(v) for v in self.x]
        self.ext = rn.RnsBasis(self.q + self.p, N)
        self.basis = self.ext.drop_last(K)
        self.key = rn.RnsHybridKey.from_channels(m.key_a, m.key_b, self.ext, ALPHA, n_special=K)
        c0 = rn.RnsPoly.from_channels(np.stack([c[0] for c in self.cts]), self.basis)
        c1 = rn.RnsPoly.from_channels(np.stack([c[1] for c in self.cts]), self.basis)
        self.ct = rn.Ciphertext(c0, c1, LOGP, self.basis.total_bits())


@pytest.fixture(scope="module")
def setup(gpu):
    return Setup(gpu)


@pytest.mark.parametrize("d,basis", sorted(MEASURED))
def test_evaluator_matches_the_cpu_plan_and_numpy(gpu, setup, d, basis):
    rn = gpu
    from rns_ntt.engine import CkksEngine

    s = setup
    coeffs = np.random.default_rng(77 + d).uniform(-1, 1, d + 1)
    plan = rn.poly_eval_plan(coeffs, basis, LOGP)
    n_lincomb = sum(op[0] == "lincomb" for op in plan.ops)
    assert plan.n_leaves <= 16 and sum(op[0] == "lincomb" and op[5] for op in plan.ops) == 1
    s.basis.profile_enable(True)
    try:
        got = CkksEngine.evaluate_polynomial_hybrid(s.ct, coeffs, s.key, basis=basis)
        launches = s.basis.profile_read("lincomb")[0]
    finally:
        s.basis.profile_enable(False)
    # all leaves from ONE launch; the Chebyshev powers add one un-rescaled launch each
    assert launches == n_lincomb == (1 if basis == "monomial" else 1 + len(plan.giants) + plan.m - 2)
    lv = L - plan.depth
    assert got.c0.basis.channel_count() == lv and got.c0.n_polys == B
    assert got.logp == LOGP and got.logq == s.ct.logq - LOGP * plan.depth
    assert not got.c0.is_ntt_domain() and not got.c1.is_ntt_domain()
    w0, w1 = got.c0.channels_batch(), got.c1.channels_batch()
    tol = 4 * MEASURED[(d, basis)]
    for b in sorted({0, B - 1}):
        r0, r1 = s.model.runner.run(plan, s.cts[b])
        assert np.array_equal(w0[b], r0), f"c0 of ciphertext {b} differs from the CPU execution of the plan"
        assert np.array_equal(w1[b], r1), f"c1 of ciphertext {b} differs from the CPU execution of the plan"
        err = float(np.max(np.abs(s.model.decode((w0[b], w1[b])) - plain_value(coeffs, basis, s.x[b]))))
        print(f"degree {d} {basis}, ciphertext {b}: decode error {err:.3e} (tolerance {tol:.3e})")
        assert err < tol


def test_evaluator_refuses_what_it_cannot_run(gpu, setup):
    rn = gpu
    from rns_ntt.engine import CkksEngine

    s = setup
    with pytest.raises(ValueError, match="levels"):  # degree 31 consumes 6 levels: 7 limbs are fine, 6 are not
        low = rn.Ciphertext(s.ct.c0.mod_drop_last(1), s.ct.c1.mod_drop_last(1), LOGP, s.ct.logq - LOGP)
        CkksEngine.evaluate_polynomial_hybrid(low, np.ones(32), s.key)
    with pytest.raises(ValueError, match="bits"):  # the consumed primes must have logp bits
        odd = rn.Ciphertext(s.ct.c0, s.ct.c1, 29, s.ct.logq)
        CkksEngine.evaluate_polynomial_hybrid(odd, [0.5, 0.25], s.key)
