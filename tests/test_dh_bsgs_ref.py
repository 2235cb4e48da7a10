"""The yardstick of the double-hoisted transform (tests/dh_bsgs_ref.py) on the
CPU at N = 2^8, pinned before any GPU run relies on it: the all-zero-steps case
is sum diag c exactly; with keys derived from a secret the result decrypts to
the matrix-vector sum within the bound the definition gives, and to the same
polynomial as bsgs_hybrid_ref within the two bounds."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from dh_bsgs_ref import dh_bsgs_ref, lift_times_p, plaintexts_over_e
from hoist_ref import rotation_exponent
from hybrid_hoist_ref import bsgs_hybrid_ref
from hybrid_ref import (crt_centered, digit_limbs, hybrid_key_plain, lift_small, moddown_ref, n_digits)

N = 1 << 8
RINGS = [(3, 2, 2, 31), (3, 1, 1, 31), (3, 3, 3, 31), (3, 2, 2, 61)]  # (Lv, K, alpha, bits)
BABY, GIANT = [0, 1, -3], [4, 0, -8, 0]


def _sigma_int(v, k):
    g = rotation_exponent(k, N)
    out = [0] * N
    for i, c in enumerate(v):
        t = i * g % (2 * N)
        out[t % N] = -int(c) if t >= N else int(c)
    return out


def _negacyclic(a, b):
    full = np.convolve(np.asarray(a, dtype=object), np.asarray(b, dtype=object))
    out = [int(v) for v in full[:N]]
    for i, v in enumerate(full[N:]):
        out[i] -= int(v)
    return out


def _ternary(rng, h):
    s = np.zeros(N, dtype=np.int64)
    idx = rng.choice(N, size=h, replace=False)
    s[idx] = rng.choice(np.array([-1, 1]), size=h)
    return s


def _rot_key(Be, mod, Lv, alpha, s, k, rng, sigma=3.2):
    """The hybrid rotation key of step k (target sigma_k(s)): b_d = -a_d s + e_d
    + G_d over E.  Returns key_a, key_b, max |e_d|."""
    beta = n_digits(Lv, alpha)
    sE = lift_small(s, mod)
    G = hybrid_key_plain(mod, Lv, alpha, lift_small(np.array(_sigma_int(s, k), dtype=np.int64), mod[:Lv]))
    key_a = orc.uniform_poly(mod, N, rng, batch=beta)
    key_b = np.zeros_like(key_a)
    emax = 0
    for d in range(beta):
        e = np.rint(rng.normal(0, sigma, N)).astype(np.int64)
        emax = max(emax, int(np.max(np.abs(e))))
        b = orc.add(Be, orc.neg(Be, orc.mul(Be, key_a[d], sE)), lift_small(e, mod))
        key_b[d] = orc.add(Be, b, G[d])
    return key_a, key_b, emax


def _ks_term(mod, Lv, alpha, emax):
    """N sum_d |I_d| Q_d max|e_d| / P + 1: the key-error term of one hybrid
    key-switch after the division by P (tests/test_hybrid_ref.py's _bound)."""
    P = 1
    for p in mod[Lv:]:
        P *= p
    tot = 0
    for d in range(n_digits(Lv, alpha)):
        I = list(digit_limbs(Lv, alpha, d))
        Qd = 1
        for i in I:
            Qd *= mod[i]
        tot += len(I) * Qd
    return N * tot * emax // P + 1


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_all_zero_steps_is_the_plain_sum_exactly(Lv, K, alpha, bits):
    """ModDown(P x) = x: with every step 0 no key is read and the result is
    sum_ji diag_ji c, word for word -- for random words and for the all-(q - 1)
    ciphertext against all-(m - 1) plaintexts."""
    mod = orc.generate_primes(bits, Lv + K, N)
    Bc, Be = orc.Basis(mod[:Lv], N), orc.Basis(mod, N)
    rng = np.random.default_rng(400 + Lv + K)
    x = orc.uniform_poly(mod[:Lv], N, rng)
    assert np.array_equal(moddown_ref(mod, Lv, lift_times_p(mod, Lv, x)), x)
    for edge in (False, True):
        c0, c1 = orc.uniform_poly(mod[:Lv], N, rng), orc.uniform_poly(mod[:Lv], N, rng)
        plain = [rng.integers(-(1 << 20), 1 << 20, N) for _ in range(4)]
        dE = plaintexts_over_e(plain, mod)
        if edge:
            c0[:] = c1[:] = np.array(mod[:Lv], dtype=np.uint64)[:, None] - np.uint64(1)
            dE[:] = np.array(mod, dtype=np.uint64)[None, :, None] - np.uint64(1)  # the integer -1 mod every modulus
        o0, o1 = dh_bsgs_ref(Bc, Be, c0, c1, [0, 0], [0, 0], dE, [None, None], [None, None], alpha)
        w0 = w1 = None
        for t in range(4):
            p0, p1 = orc.mul(Bc, c0, dE[t][:Lv]), orc.mul(Bc, c1, dE[t][:Lv])
            w0 = p0 if w0 is None else orc.add(Bc, w0, p0)
            w1 = p1 if w1 is None else orc.add(Bc, w1, p1)
        assert np.array_equal(o0, w0) and np.array_equal(o1, w1), edge


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS[:1] + RINGS[3:])
def test_naive_products_give_the_same_words(Lv, K, alpha, bits):
    mod = orc.generate_primes(bits, Lv + K, N)
    Bc, Be = orc.Basis(mod[:Lv], N), orc.Basis(mod, N)
    rng = np.random.default_rng(410)
    beta = n_digits(Lv, alpha)
    c0, c1 = orc.uniform_poly(mod[:Lv], N, rng), orc.uniform_poly(mod[:Lv], N, rng)
    baby, giant = [0, 1], [2, 0]
    bk = [None, (orc.uniform_poly(mod, N, rng, batch=beta), orc.uniform_poly(mod, N, rng, batch=beta))]
    gk = [(orc.uniform_poly(mod, N, rng, batch=beta), orc.uniform_poly(mod, N, rng, batch=beta)), None]
    dE = orc.uniform_poly(mod, N, rng, batch=4)
    a = dh_bsgs_ref(Bc, Be, c0, c1, baby, giant, dE, bk, gk, alpha)
    b = dh_bsgs_ref(Bc, Be, c0, c1, baby, giant, dE, bk, gk, alpha, mul=lambda u, v: orc.mul_naive(Be, u, v))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("seed", [420, 421])
@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_decrypts_to_the_matrix_vector_sum_and_as_bsgs_hybrid_ref_does(Lv, K, alpha, bits, seed):
    """out0 + out1 s = sum_j sigma_{g_j}(sum_i p_ji sigma_{b_i}(m)) + error.

    The bound, from the definition.  Write B1(e) = N sum_d |I_d| Q_d e / P + 1,
    the key-error term of one key-switch after the division by P.  A rotating
    baby's pair (T0_i, T1_i) decrypts under sigma^-1(s) to P (c0 + c1 s) plus
    the key-error sum, exactly over E -- nothing is rounded -- so Vt_j carries
    sum_i |p_ji|_1 P B1(e_i).  A rotating giant rounds once, W_j = (Vt1_j -
    delta) / P with 0 <= delta < K P per coefficient, which costs K |s|_1
    after the final division, and adds its own key error B1(e_gj).  The final
    ModDown of the pair costs (K + 1)(1 + |s|_1) as in tests/test_hybrid_ref.py:

        error <= sum_j sum_{b_i != 0} |p_ji|_1 B1(e_i) + sum_{g_j != 0} (B1(e_gj) + K |s|_1)
                 + (K + 1)(1 + |s|_1)

    bsgs_hybrid_ref's own bound has, for every rotating baby, the whole
    key-switch bound B1 + (K + 1)(1 + |s|_1) multiplied by |p_ji|_1 (its baby
    ModDown roundings meet the plaintexts).  Both are asserted, and the two
    results agree as decryptions within the sum of the two."""
    mod = orc.generate_primes(bits, Lv + K, N)
    modc = mod[:Lv]
    Bc, Be = orc.Basis(modc, N), orc.Basis(mod, N)
    rng = np.random.default_rng(seed)
    s = _ternary(rng, N // 2)
    s1 = int(np.sum(np.abs(s)))
    m = rng.integers(-(1 << 12), 1 << 12, N)
    c1 = orc.uniform_poly(modc, N, rng)
    e = np.rint(rng.normal(0, 3.2, N)).astype(np.int64)
    me = m + e
    c0 = orc.add(Bc, orc.neg(Bc, orc.mul(Bc, c1, lift_small(s, modc))), lift_small(me, modc))
    n1 = len(BABY)
    bk3 = [None if b == 0 else _rot_key(Be, mod, Lv, alpha, s, b, rng) for b in BABY]
    gk3 = [None if g == 0 else _rot_key(Be, mod, Lv, alpha, s, g, rng) for g in GIANT]
    bk = [None if k is None else k[:2] for k in bk3]
    gk = [None if k is None else k[:2] for k in gk3]
    pl = [rng.integers(-8, 9, N) for _ in range(n1 * len(GIANT))]
    dE = plaintexts_over_e(pl, mod)
    o0, o1 = dh_bsgs_ref(Bc, Be, c0, c1, BABY, GIANT, dE, bk, gk, alpha)
    r0, r1 = bsgs_hybrid_ref(Bc, Be, c0, c1, BABY, GIANT, [d[:Lv] for d in dE], bk, gk, alpha)
    assert not np.array_equal(o0, r0) and not np.array_equal(o1, r1)  # not that call's words

    def decrypt(a0, a1):
        return crt_centered(orc.add(Bc, a0, orc.mul(Bc, a1, lift_small(s, modc))), modc)

    want = [0] * N
    for j, g in enumerate(GIANT):
        v = [0] * N
        for i, b in enumerate(BABY):
            r = _sigma_int(me, b) if b else [int(x) for x in me]
            v = [x + y for x, y in zip(v, _negacyclic(pl[j * n1 + i], r))]
        v = _sigma_int(v, g) if g else v
        want = [x + y for x, y in zip(want, v)]
    got_dh, got_old = decrypt(o0, o1), decrypt(r0, r1)
    err_dh = max(abs(a - b) for a, b in zip(got_dh, want))
    err_old = max(abs(a - b) for a, b in zip(got_old, want))
    md = (K + 1) * (1 + s1)
    bound_dh, bound_old = md, md
    for j, g in enumerate(GIANT):
        for i, k3 in enumerate(bk3):
            if k3 is not None:
                p1 = int(np.sum(np.abs(pl[j * n1 + i])))
                bound_dh += p1 * _ks_term(mod, Lv, alpha, k3[2])
                bound_old += p1 * (_ks_term(mod, Lv, alpha, k3[2]) + md)
        if gk3[j] is not None:
            bound_dh += _ks_term(mod, Lv, alpha, gk3[j][2]) + K * s1
            bound_old += _ks_term(mod, Lv, alpha, gk3[j][2])
    both = max(abs(a - b) for a, b in zip(got_dh, got_old))
    print(f"Lv={Lv} K={K} alpha={alpha} bits={bits} seed={seed}: double-hoisted error {err_dh} (bound {bound_dh}), "
          f"rnt_ct_linear_bsgs_hybrid's {err_old} (bound {bound_old}), between the two {both}")
    assert err_dh <= bound_dh
    assert err_old <= bound_old
    assert both <= bound_dh + bound_old
