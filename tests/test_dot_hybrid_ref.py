"""The yardstick of the hybrid inner product (tests/dot_hybrid_ref.py) pinned on
the CPU: one term is the hybrid multiply's yardstick, the order of the terms
does not matter, and with a drawn key the result decrypts to sum_i m_i m'_i
with the error of ONE key-switch."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from dot_hybrid_ref import dot_relin_hybrid_ref, dot_relin_rescale_hybrid_ref, dot_tensor_ref
from hybrid_ref import crt_centered, lift_small, mul_relin_hybrid_ref, n_digits
from hybrid_rescale_ref import mul_relin_rescale_hybrid_ref
from test_hybrid_ref import N, _bound, _hybrid_keys, _log2, _moduli, _ternary

RINGS = [(3, 2, 2, 31), (3, 1, 1, 31), (4, 2, 3, 31), (3, 2, 2, 61)]  # Lv, K, alpha, bits


def _case(Lv, K, alpha, bits, n_terms, seed):
    mod = _moduli(Lv, K, bits)
    rng = np.random.default_rng(seed)
    Bc, Be = orc.Basis(mod[:Lv], N), orc.Basis(mod, N)
    ins = [orc.uniform_poly(mod[:Lv], N, rng, batch=n_terms) for _ in range(4)]
    beta = n_digits(Lv, alpha)
    ka, kb = orc.uniform_poly(mod, N, rng, batch=beta), orc.uniform_poly(mod, N, rng, batch=beta)
    return mod, Bc, Be, ins, ka, kb


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_one_term_is_the_hybrid_multiply(Lv, K, alpha, bits):
    mod, Bc, Be, (x0, x1, y0, y1), ka, kb = _case(Lv, K, alpha, bits, 1, 7 * Lv + alpha)
    got = dot_relin_hybrid_ref(Bc, Be, x0, x1, y0, y1, ka, kb, alpha)
    want = mul_relin_hybrid_ref(Bc, Be, x0[0], x1[0], y0[0], y1[0], ka, kb, alpha)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    got = dot_relin_rescale_hybrid_ref(Bc, Be, x0, x1, y0, y1, ka, kb, alpha)
    want = mul_relin_rescale_hybrid_ref(Bc, Be, x0[0], x1[0], y0[0], y1[0], ka, kb, alpha)
    assert got[0].shape == (Lv - 1, N)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_invariant_under_a_permutation_of_the_terms(Lv, K, alpha, bits):
    n_terms = 5
    mod, Bc, Be, ins, ka, kb = _case(Lv, K, alpha, bits, n_terms, 11 * Lv + alpha)
    perm = np.random.default_rng(3).permutation(n_terms)
    assert not np.array_equal(perm, np.arange(n_terms))
    for fn in (dot_relin_hybrid_ref, dot_relin_rescale_hybrid_ref):
        a = fn(Bc, Be, *ins, ka, kb, alpha)
        b = fn(Bc, Be, *[x[perm] for x in ins], ka, kb, alpha)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        q = np.array(mod[: a[0].shape[0]], dtype=np.uint64)[:, None]
        assert (a[0] < q).all() and (a[1] < q).all()
    # more than one term is NOT the sum of the hybrid multiplies: ModUp and ModDown of a sum are not the sums
    x0, x1, y0, y1 = ins
    tot = None
    for i in range(n_terms):
        m = mul_relin_hybrid_ref(Bc, Be, x0[i], x1[i], y0[i], y1[i], ka, kb, alpha)
        tot = m if tot is None else (orc.add(Bc, tot[0], m[0]), orc.add(Bc, tot[1], m[1]))
    one = dot_relin_hybrid_ref(Bc, Be, *ins, ka, kb, alpha)
    assert not np.array_equal(one[0], tot[0])


def _negacyclic_square(s):
    n = len(s)
    full = np.convolve(s.astype(np.int64), s.astype(np.int64))
    out = full[:n].copy()
    out[: n - 1] -= full[n:]
    return out


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
@pytest.mark.parametrize("n_terms", [1, 6])
def test_decrypts_to_the_sum_of_products_with_one_key_switch_error(Lv, K, alpha, bits, n_terms):
    """Noise-free encryptions x0_i = m_i - x1_i s of small messages under a
    ternary s and a drawn relinearisation key for s^2: out0 + out1 s -
    sum_i m_i m'_i is the error of the one key-switch of d2, within the bound
    test_hybrid_ref.py derives for one key-switch however many terms."""
    mod = _moduli(Lv, K, bits)
    modc = mod[:Lv]
    rng = np.random.default_rng(100 * Lv + 10 * alpha + n_terms)
    Bc, Be = orc.Basis(modc, N), orc.Basis(mod, N)
    s = _ternary(rng, N, N // 2)
    s2 = _negacyclic_square(s)
    key_a, key_b, emax = _hybrid_keys(Be, mod, Lv, alpha, s, s2, rng)
    sC = lift_small(s, modc)

    def encrypt(m):
        c1 = orc.uniform_poly(modc, N, rng)
        return orc.add(Bc, lift_small(m, modc), orc.neg(Bc, orc.mul(Bc, c1, sC))), c1

    msgs = rng.integers(-50, 51, size=(2, n_terms, N))
    cx = [encrypt(m) for m in msgs[0]]
    cy = [encrypt(m) for m in msgs[1]]
    x0, x1 = np.stack([c[0] for c in cx]), np.stack([c[1] for c in cx])
    y0, y1 = np.stack([c[0] for c in cy]), np.stack([c[1] for c in cy])
    out0, out1 = dot_relin_hybrid_ref(Bc, Be, x0, x1, y0, y1, key_a, key_b, alpha)
    want = None
    for mx, my in zip(msgs[0], msgs[1]):
        p = orc.mul(Bc, lift_small(mx, modc), lift_small(my, modc))
        want = p if want is None else orc.add(Bc, want, p)
    dec = orc.add(Bc, out0, orc.mul(Bc, out1, sC))
    err = max(abs(v) for v in crt_centered(orc.add(Bc, dec, orc.neg(Bc, want)), modc))
    bound = _bound(mod, Lv, K, alpha, emax, s)
    print(f"Lv={Lv} K={K} alpha={alpha} bits={bits} terms={n_terms}: error {err} (2^{_log2(err):.1f}), bound {bound}")
    assert err <= bound
    # the tensor alone decrypts exactly: d0 + d1 s + d2 s^2 = sum_i m_i m'_i
    d0, d1, d2 = dot_tensor_ref(Bc, x0, x1, y0, y1)
    s2C = lift_small(s2, modc)
    exact = orc.add(Bc, orc.add(Bc, d0, orc.mul(Bc, d1, sC)), orc.mul(Bc, d2, s2C))
    assert np.array_equal(exact, want)
