"""Inner sums over slots at the engine level (CkksEngine.inner_sum_hybrid over
rotsum_plan and rnt_ct_rotsum_hybrid): N = 2^10, 4 x 30-bit limbs + 2 special
primes, alpha = 2, scale 2^30; encode -> encrypt -> inner sum -> decrypt ->
decode against numpy's sum of the rotated slot vectors, with the level and the
scale unchanged."""
from __future__ import annotations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, L, K, ALPHA, LOGP = 1024, 4, 2, 2, 30
# tools/rotsum_tolerance.py, eight seeds, this ring: the largest decode error of
# the EXISTING chain of rotate_ciphertext_hybrid + add_ciphertexts over the
# configurations below (profiles/rotsum_tolerance.txt).  The new call is
# allowed 4 x that: both are sums of independent key-switch errors of one
# distribution and the new call has fewer ModDown terms, so anything beyond
# that factor is a defect.
CHAIN_ERR_MEASURED = 3.349e-04

# n, stride, plan arguments
CASES = [
    (16, 1, {"radix": 2}),
    (16, 1, {"radix": 4}),
    (16, 1, {"radix": 16}),
    (16, 4, {"radix": 4}),
    (12, 1, {"radices": (4, 3)}),
]


@pytest.fixture(scope="module")
def world(gpu):
    """One engine, secret, ciphertext and slot vector for every case."""
    from rns_ntt.engine import CkksEngine

    rn = gpu
    eng = CkksEngine(rn.generate_primes(30, L, N), N, error_std=3.2, hamming_weight=N // 2,
                     special_moduli=rn.generate_primes(31, K, N))
    rng = rn.DeviceRng(7301)
    sk = eng.generate_secret_key(rng)
    pk = eng.generate_public_key(sk, rng)
    x = np.random.default_rng(7302).uniform(-1, 1, N // 2)
    enc = rn.CkksEncoder(N, LOGP)
    ct = eng.encrypt(enc.encode(x, eng.basis), pk, rng)
    return rn, CkksEngine, eng, rng, sk, enc, ct, x


@pytest.mark.parametrize("n,stride,kw", CASES, ids=[f"n{n}-s{s}-{list(kw.values())[0]}" for n, s, kw in CASES])
def test_inner_sum_decodes_to_the_sum_of_rotated_slots(world, n, stride, kw):
    rn, CkksEngine, eng, rng, sk, enc, ct, x = world
    plan = rn.rotsum_plan(n, stride, n_slots=N // 2, **kw)
    sets = eng.generate_rotsum_key_sets(sk, plan, rng, ALPHA)
    assert [ks.steps for ks in sets] == plan.stages and not any(ks.hoisted for ks in sets)
    before0, before1 = ct.c0.channels(), ct.c1.channels()
    out = CkksEngine.inner_sum_hybrid(ct, plan, sets)
    assert out is not ct and np.array_equal(ct.c0.channels(), before0) and np.array_equal(ct.c1.channels(), before1)
    assert out.logp == ct.logp and out.logq == ct.logq  # no scale spent
    assert out.c0.basis is ct.c0.basis and out.c0.n_polys == 1  # no level spent
    got = enc.decode(CkksEngine.decrypt_plaintext(out, CkksEngine.secret_on(sk, out.c0.basis)))
    want = sum(np.roll(x, -t * stride) for t in range(n))
    err = float(np.max(np.abs(got - want)))
    print(f"inner sum n = {n}, stride {stride}, {kw}: decode error {err:.3e}, bound {4 * CHAIN_ERR_MEASURED:.3e}")
    assert err <= 4 * CHAIN_ERR_MEASURED


def test_guards(world):
    rn, CkksEngine, eng, rng, sk, enc, ct, x = world
    plan = rn.rotsum_plan(4, 1, 2)
    sets = eng.generate_rotsum_key_sets(sk, plan, rng, ALPHA)
    with pytest.raises(ValueError, match="key sets"):
        CkksEngine.inner_sum_hybrid(ct, plan, sets[:1])
    with pytest.raises(ValueError, match="plan's steps"):
        CkksEngine.inner_sum_hybrid(ct, plan, sets[::-1])
    with pytest.raises(ValueError, match="N/2"):
        eng.generate_rotsum_key_sets(sk, rn.rotsum_plan(1024, 1, 2), rng, ALPHA)
