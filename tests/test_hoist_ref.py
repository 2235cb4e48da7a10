"""The hoisted rotation's yardstick (tests/hoist_ref.py) on the CPU: against
schoolbook products, against the regrouped form the library computes
(sigma(c0 + sum_i D_i sigma^-1(key_i)), one automorphism by g^-1 per key poly),
against orc.rotate_ciphertext (different words on the same inputs) and, with
real keys, against the decryption -- the definition is pinned here, on a host
without a GPU, before any GPU run relies on it."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest

import pyoracle as orc
from bsgs_ref import bsgs_ref
from hoist_ref import (bsgs_hoisted_ref, digits, hoisting_form_coeff, rotate_hoisted_ref, rotation_exponent)

STEPS = [1, -3, 5]
RINGS = [(6, 4, 31), (8, 3, 61)]


def _case(log_n, L, bits, seed=31):
    n = 1 << log_n
    mod = orc.generate_primes(bits, L, n)
    Bo = orc.Basis(mod, n)
    rng = np.random.default_rng(seed)
    c0, c1 = orc.uniform_poly(mod, n, rng), orc.uniform_poly(mod, n, rng)
    keys = {k: (orc.uniform_poly(mod, n, rng, batch=L), orc.uniform_poly(mod, n, rng, batch=L)) for k in STEPS}
    return Bo, mod, c0, c1, keys


@pytest.mark.parametrize("log_n,L,bits", RINGS)
def test_hoisted_ref_matches_schoolbook_products(log_n, L, bits):
    Bo, mod, c0, c1, keys = _case(log_n, L, bits)
    q = np.array(mod, dtype=np.uint64)[:, None]
    for k in STEPS:
        got = rotate_hoisted_ref(Bo, c0, c1, k, *keys[k])
        want = rotate_hoisted_ref(Bo, c0, c1, k, *keys[k], mul=lambda x, y: orc.mul_naive(Bo, x, y))
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert (got[0] < q).all() and (got[1] < q).all()


@pytest.mark.parametrize("log_n,L,bits", RINGS)
def test_hoisted_ref_equals_the_regrouped_form(log_n, L, bits):
    """out = sigma(c0 + sum_i D_i sigma^-1(key_b[i])), sigma(sum_i D_i sigma^-1(key_a[i]))."""
    Bo, mod, c0, c1, keys = _case(log_n, L, bits, seed=32)
    n = 1 << log_n
    D = digits(Bo, c1)
    for k in STEPS:
        ka, kb = keys[k]
        ha, hb = hoisting_form_coeff(Bo, ka, k), hoisting_form_coeff(Bo, kb, k)
        s0, s1 = c0, None
        for i in range(L):
            s0 = orc.add(Bo, s0, orc.mul(Bo, D[i], hb[i]))
            p = orc.mul(Bo, D[i], ha[i])
            s1 = p if s1 is None else orc.add(Bo, s1, p)
        g = rotation_exponent(k, n)
        want = rotate_hoisted_ref(Bo, c0, c1, k, ka, kb)
        assert np.array_equal(orc.automorphism(Bo, s0, g)[0], want[0]), k
        assert np.array_equal(orc.automorphism(Bo, s1, g)[0], want[1]), k
        # the automorphism by g is rotate_slots, the negative step's composition included
        assert np.array_equal(orc.automorphism(Bo, c0, g)[0], orc.rotate_slots(Bo, c0, k)[0]), k


@pytest.mark.parametrize("log_n,L,bits", RINGS)
def test_hoisted_words_differ_from_rotate_ciphertext(log_n, L, bits):
    Bo, mod, c0, c1, keys = _case(log_n, L, bits, seed=33)
    for k in STEPS:
        h = rotate_hoisted_ref(Bo, c0, c1, k, *keys[k])
        p = orc.rotate_ciphertext(Bo, c0, c1, k, *keys[k])
        assert not np.array_equal(h[0], p[0]) and not np.array_equal(h[1], p[1]), k


def test_step_zero_is_the_identity():
    Bo, mod, c0, c1, keys = _case(6, 4, 31, seed=34)
    o0, o1 = rotate_hoisted_ref(Bo, c0, c1, 0, None, None)
    assert np.array_equal(o0, c0) and np.array_equal(o1, c1)


def test_bsgs_hoisted_ref_schoolbook_and_zero_babies():
    """Schoolbook products give the same words; with every baby step 0 no
    rotation is hoisted and the yardstick is tests/bsgs_ref.py's."""
    Bo, mod, c0, c1, keys = _case(6, 2, 31, seed=35)
    n, L = 64, 2
    rng = np.random.default_rng(36)
    baby, giant = [0, 1, -3, 1], [0, 4]
    bk = [None if b == 0 else keys[b] for b in baby]
    gk = [None, (orc.uniform_poly(mod, n, rng, batch=L), orc.uniform_poly(mod, n, rng, batch=L))]
    diag = orc.uniform_poly(mod, n, rng, batch=len(baby) * len(giant))
    got = bsgs_hoisted_ref(Bo, c0, c1, baby, giant, diag, bk, gk)
    want = bsgs_hoisted_ref(Bo, c0, c1, baby, giant, diag, bk, gk, mul=lambda x, y: orc.mul_naive(Bo, x, y))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    plain = bsgs_ref(Bo, c0, c1, baby, giant, diag, bk, gk)
    assert not np.array_equal(got[0], plain[0])
    z = [0, 0]
    d2 = diag[: len(z) * len(giant)]
    a = bsgs_hoisted_ref(Bo, c0, c1, z, giant, d2, [None, None], gk)
    b = bsgs_ref(Bo, c0, c1, z, giant, d2, [None, None], gk)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_hoisted_rotation_decrypts_to_the_rotated_slots():
    """Real keys (tools/hoist_tolerance.py's construction) at N = 64: the
    decode error of the yardstick stays under the 1e-3 asked of the
    parameters, as the plain rotation's does."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import hoist_tolerance as ht

    for seed in (0, 1):
        errs = ht.run_rotations(seed)
        assert errs["hoisted"] < 1e-3 and errs["plain"] < 1e-3, errs
