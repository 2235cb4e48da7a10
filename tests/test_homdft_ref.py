"""The CPU model of ModRaise and the coefficient/slot transforms
(tests/homdft_ref.py) pinned without a GPU: mod_raise_ref against the
Garner-digit formulation the kernel uses, the exact ModRaise identity, and the
raise -> CoeffToSlot -> SlotToCoeff pipeline inside the measured tolerance.

MEASURED: tools/homdft_tolerance.py (profiles/homdft_tolerance.txt), eight
seeds, (N, depth, order) -> (slot-side, round-trip) largest decode error at
2^20; the tolerance is 4 x, the project's standing margin."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from homdft_ref import (HomDftModel, mod_raise_garner_ref, mod_raise_ref, mul_monomial_ref, run_pipeline)
from rns_ntt.homdft import homdft_plan

MEASURED = {(256, 3, "bitrev"): (1.322e-03, 1.098e-02), (1024, 3, "bitrev"): (5.916e-03, 8.171e-02),
            (256, 1, "natural"): (4.269e-03, None)}
L, K, ALPHA, LOGP, HAMMING = 7, 2, 2, 20, 32


def planted(q, n, rng):
    """Uniform residues with 0, 1, Q0 - 1, floor(Q0/2), floor(Q0/2) + 1 and
    the all-(q_i - 1) vector at coefficients 0, 1, N - 1, 2, 3, N - 2."""
    Q0 = 1
    for v in q:
        Q0 *= v
    x = orc.uniform_poly(q, n, rng)
    vals = [[v % m for m in q] for v in (0, 1, Q0 - 1, Q0 // 2, Q0 // 2 + 1)] + [[m - 1 for m in q]]
    for pos, r in zip((0, 1, n - 1, 2, 3, n - 2), vals):
        x[:, pos] = r
    return x, Q0


@pytest.mark.parametrize("bits", [31, 61, "mixed"])
@pytest.mark.parametrize("l0", [1, 2, 3, 4])
def test_mod_raise_ref_matches_the_garner_formulation(l0, bits):
    n, Lout = 64, 7
    if bits == "mixed":
        a, b = orc.generate_primes(40, Lout, n), orc.generate_primes(61, Lout, n)
        mod = [(a if i % 2 == 0 else b)[i // 2] for i in range(Lout)]
    else:
        mod = orc.generate_primes(bits, Lout, n)
    x, Q0 = planted(mod[:l0], n, np.random.default_rng(l0))
    want = mod_raise_ref(x, mod[:l0], mod)
    assert np.array_equal(want, mod_raise_garner_ref(x, mod[:l0], mod))
    assert np.array_equal(want[:l0], x)
    # the planted values, limb l0: 0, 1, -1, floor(Q0/2), floor(Q0/2) + 1 - Q0, -1
    q = mod[l0]
    assert [int(v) for v in want[l0, [0, 1, n - 1, 2, 3, n - 2]]] == \
        [0, 1, q - 1, (Q0 // 2) % q, (Q0 // 2 + 1 - Q0) % q, q - 1]


def test_mul_monomial_ref_is_the_ring_product():
    n = 32
    mod = orc.generate_primes(31, 2, n)
    Bo = orc.Basis(mod, n)
    x = orc.uniform_poly(mod, n, np.random.default_rng(2))
    x[:, ::3] = 0
    for k in (0, 1, n - 1, n, n + 5, 2 * n - 1, -1, 2 * n + 3):
        e = np.zeros(n, dtype=np.int64)
        kk = k % (2 * n)
        e[kk % n] = 1 if kk < n else -1
        assert np.array_equal(mul_monomial_ref(x, mod, k), orc.mul(Bo, x, orc.from_coeffs(Bo, e))), k


@pytest.fixture(scope="module")
def pipeline():
    n = 256
    q, p = orc.generate_primes(30, L, n), orc.generate_primes(31, K, n)
    model = HomDftModel(q, p, n, ALPHA, HAMMING, seed=2024)
    values = model.rng.uniform(-1, 1, n // 2) + 1j * model.rng.uniform(-1, 1, n // 2)
    r = run_pipeline(model, homdft_plan(n, "coeff_to_slot", 3), homdft_plan(n, "slot_to_coeff", 3), values, LOGP)
    return model, values, r


def test_mod_raise_identity(pipeline):
    """t - m = Q0 I with |I| <= (h + 1) / 2 coefficient-wise: m the centred
    decryption on one limb, t on the raised basis."""
    model, _, r = pipeline
    m, t, Q0 = model.decrypt(r["first"]), r["a"], model.q[0]
    assert all((u - v) % Q0 == 0 for u, v in zip(t, m))
    assert max(abs((u - v) // Q0) for u, v in zip(t, m)) <= (HAMMING + 1) / 2
    assert any(u != v for u, v in zip(t, m))  # the raise does add a multiple of Q0 somewhere


def test_pipeline_is_inside_the_measured_tolerance(pipeline):
    model, values, r = pipeline
    slot, back = MEASURED[(256, 3, "bitrev")]
    print(f"slot-side error {r['slot_err']:.3e} (tolerance {4 * slot:.3e}), round trip {r['back_err']:.3e} "
          f"(tolerance {4 * back:.3e})")
    assert r["slot"][0].shape[0] == L - 3 and r["back"][0].shape[0] == 1
    assert r["slot_err"] < 4 * slot
    assert r["back_err"] < 4 * back
    # and the message itself comes back: the one-limb decryption decodes to the input slots
    assert np.max(np.abs(model.decode(r["back"], LOGP) - values)) < 4 * back + 1e-3
