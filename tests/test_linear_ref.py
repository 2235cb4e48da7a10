"""The linear transform's CPU yardstick (tests/lt_ref.py) against a version
whose plaintext products are schoolbook, at N = 16 with two 31-bit primes:
the yardstick is shown right here, before any GPU run compares against it."""
from __future__ import annotations

import numpy as np

import pyoracle as orc
from lt_ref import linear_ref

STEPS = [0, 1, -3, 5, 1]


def _case(seed=11):
    n, L = 16, 2
    mod = orc.generate_primes(31, L, n)
    Bo = orc.Basis(mod, n)
    rng = np.random.default_rng(seed)
    c0, c1 = orc.uniform_poly(mod, n, rng), orc.uniform_poly(mod, n, rng)
    diag = orc.uniform_poly(mod, n, rng, batch=len(STEPS))
    keys = [None if k == 0 else (orc.uniform_poly(mod, n, rng, batch=L), orc.uniform_poly(mod, n, rng, batch=L))
            for k in STEPS]
    return Bo, mod, c0, c1, diag, keys


def test_linear_ref_matches_schoolbook_products():
    Bo, mod, c0, c1, diag, keys = _case()
    got = linear_ref(Bo, c0, c1, STEPS, diag, keys)
    want = linear_ref(Bo, c0, c1, STEPS, diag, keys, mul=lambda x, y: orc.mul_naive(Bo, x, y))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    q = np.array(mod, dtype=np.uint64)[:, None]
    assert (got[0] < q).all() and (got[1] < q).all()


def test_linear_ref_step_zero_is_the_plain_product():
    Bo, mod, c0, c1, diag, keys = _case(12)
    o0, o1 = linear_ref(Bo, c0, c1, [0], diag[:1], [None])
    assert np.array_equal(o0, orc.mul_naive(Bo, c0, diag[0]))
    assert np.array_equal(o1, orc.mul_naive(Bo, c1, diag[0]))


def test_linear_ref_is_linear_in_the_terms():
    """The sum over all terms equals the sum of the one-term transforms."""
    Bo, mod, c0, c1, diag, keys = _case(13)
    full = linear_ref(Bo, c0, c1, STEPS, diag, keys)
    acc = None
    for t, k in enumerate(STEPS):
        one = linear_ref(Bo, c0, c1, [k], diag[t:t + 1], [keys[t]])
        acc = one if acc is None else (orc.add(Bo, acc[0], one[0]), orc.add(Bo, acc[1], one[1]))
    assert np.array_equal(full[0], acc[0]) and np.array_equal(full[1], acc[1])
