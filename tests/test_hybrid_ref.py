"""The hybrid key-switch's yardstick (tests/hybrid_ref.py) on the CPU: ModUp
and ModDown against big-integer CRT, the ring products against schoolbook, and
with drawn keys the decryption error against the bound that follows from the
definition -- pinned here, on a host without a GPU, before any GPU run relies
on it."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from hybrid_ref import (crt_centered, digit_limbs, hybrid_key_plain, keyswitch_hybrid_ref, lift_small, moddown_ref,
                        modup_ref, n_digits, restrict_key)

N = 32
# (Lv, K, bits); the last six are the rings of tests/test_gpu_hybrid_tiers.py's
# register tiers (Lv = alpha + 1, K = alpha at alpha = 5, 9, 17)
RINGS = [(3, 2, 31), (4, 2, 31), (3, 2, 61), (5, 1, 31),
         (6, 5, 31), (10, 9, 31), (18, 17, 31), (6, 5, 61), (10, 9, 61), (18, 17, 61)]
# (alpha, K, bits) of the GPU tier matrix: both edges of every register tier of
# k_modup / k_moddown and the generic form, with Lv = alpha + 1
TIERS = [(a, a, bits) for a in (4, 5, 8, 9, 16, 17) for bits in (31, 61)]


def _moduli(Lv, K, bits, n=N):
    mod = orc.generate_primes(bits, Lv + K, n)
    return mod  # the first Lv are the q_i, the rest the special primes


def _crt_nonneg(residues, moduli):
    Q = 1
    for m in moduli:
        Q *= int(m)
    return [v % Q for v in crt_centered(residues, moduli)], Q


@pytest.mark.parametrize("Lv,K,bits", RINGS)
def test_modup_is_the_residue_plus_a_small_multiple_of_the_digit_modulus(Lv, K, bits):
    mod = _moduli(Lv, K, bits)
    rng = np.random.default_rng(1)
    x = orc.uniform_poly(mod[:Lv], N, rng)
    x[:, 0] = [m - 1 for m in mod[:Lv]]  # the largest residues too
    for alpha in sorted({1, 2, Lv} | {a for a in (5, 9, 17) if a < Lv}):
        for d in range(n_digits(Lv, alpha)):
            I = list(digit_limbs(Lv, alpha, d))
            Qd = 1
            for i in I:
                Qd *= mod[i]
            up = modup_ref(mod, Lv, alpha, d, x)
            assert up.shape == (Lv + K, N)
            for t in I:  # the digit's own limbs are copied
                assert np.array_equal(up[t], x[t])
            full, QP = _crt_nonneg(up, mod)
            xd, _ = _crt_nonneg(x[I], [mod[i] for i in I])
            assert QP > len(I) * Qd
            for c in range(N):
                u, r = divmod(full[c] - xd[c], Qd)
                assert r == 0 and 0 <= u < len(I), (alpha, d, c, u, r)


def _below(rng, M):
    """A draw from [0, M) whose bits reach the top of M (M of any size)."""
    v = 0
    for _ in range(M.bit_length() // 62 + 2):
        v = (v << 62) | int(rng.integers(0, 1 << 62))
    return v % M


@pytest.mark.parametrize("Lv,K,bits", RINGS)
def test_moddown_divides_by_p(Lv, K, bits):
    """A = P m + r with 0 <= r < P: the fast conversion of [A]_P is r + v P with
    0 <= v < K, so ModDown returns m - v mod Q."""
    mod = _moduli(Lv, K, bits)
    rng = np.random.default_rng(2)
    Q = 1
    for m in mod[:Lv]:
        Q *= m
    P = 1
    for p in mod[Lv:]:
        P *= p
    ms = [_below(rng, Q) for _ in range(N)]
    rs = [_below(rng, P) for _ in range(N)]
    ms[0], rs[0] = Q - 1, P - 1
    ms[1], rs[1] = 0, 0
    A = np.array([[(P * m + r) % int(q) for m, r in zip(ms, rs)] for q in mod], dtype=np.uint64)
    out = moddown_ref(mod, Lv, A)
    got, _ = _crt_nonneg(out, mod[:Lv])
    for c in range(N):
        v = (ms[c] - got[c]) % Q
        assert 0 <= v < K, (c, v)
    assert got[1] == 0


@pytest.mark.parametrize("alpha,K,bits", TIERS)
def test_plain_key_of_one_switches_to_the_input(alpha, K, bits):
    """key_b = the plaintexts G_d of the target 1 (limb t of G_d is [P]_{q_t}
    on the digit's own limbs, zero elsewhere), key_a = 0: A0 = P x on the
    ciphertext limbs and 0 on the special ones, so z = 0 and the key-switch
    returns (x, 0) exactly -- for a random x and for the all-(q - 1) one.  The
    GPU tier tests assert the same identity on the device."""
    Lv = alpha + 1
    mod = _moduli(Lv, K, bits)
    Be = orc.Basis(mod, N)
    one = np.zeros((Lv, N), dtype=np.uint64)
    one[:, 0] = 1
    key_b = hybrid_key_plain(mod, Lv, alpha, one)
    assert key_b.shape == (2, Lv + K, N)
    P = 1
    for p in mod[Lv:]:
        P *= p
    for d in range(2):  # one-hot rows: [P]_{q_t} at coefficient 0 of the digit's limbs, zero elsewhere
        want = np.zeros((Lv + K, N), dtype=np.uint64)
        for t in digit_limbs(Lv, alpha, d):
            want[t, 0] = P % mod[t]
        assert np.array_equal(key_b[d], want)
    key_a = np.zeros_like(key_b)
    rng = np.random.default_rng(3 * alpha + bits)
    x = orc.uniform_poly(mod[:Lv], N, rng)
    top = np.broadcast_to(np.array(mod[:Lv], dtype=np.uint64)[:, None] - np.uint64(1), (Lv, N)).copy()
    for v in (x, top):
        acc0, acc1 = keyswitch_hybrid_ref(Be, Lv, v, key_a, key_b, alpha)
        assert np.array_equal(acc0, v) and not acc1.any()


def _log2(v):
    import math

    return math.log2(max(int(v), 1))


def _ternary(rng, n, h):
    s = np.zeros(n, dtype=np.int64)
    idx = rng.choice(n, size=h, replace=False)
    s[idx] = rng.choice(np.array([-1, 1]), size=h)
    return s


def _hybrid_keys(Be, mod, Lv, alpha, s, sp, rng, sigma=3.2):
    """Drawn a_d, e_d and b_d = -a_d s + e_d + G_d over E; returns key_a, key_b,
    max |e_d|."""
    beta = n_digits(Lv, alpha)
    sE = lift_small(s, mod)
    G = hybrid_key_plain(mod, Lv, alpha, lift_small(sp, mod[:Lv]))
    key_a = orc.uniform_poly(mod, N, rng, batch=beta)
    key_b = np.zeros_like(key_a)
    emax = 0
    for d in range(beta):
        e = np.rint(rng.normal(0, sigma, N)).astype(np.int64)
        emax = max(emax, int(np.max(np.abs(e))))
        b = orc.add(Be, orc.neg(Be, orc.mul(Be, key_a[d], sE)), lift_small(e, mod))
        key_b[d] = orc.add(Be, b, G[d])
    return key_a, key_b, emax


def _decrypt_error(Bc, modc, acc0, acc1, x, s, sp):
    sC, spC = lift_small(s, modc), lift_small(sp, modc)
    lhs = orc.add(Bc, acc0, orc.mul(Bc, acc1, sC))
    diff = orc.add(Bc, lhs, orc.neg(Bc, orc.mul(Bc, x, spC)))
    return max(abs(v) for v in crt_centered(diff, modc))


def _bound(mod, Lv, K, alpha, emax, s):
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
    return N * tot * emax // P + 1 + (K + 1) * (1 + int(np.sum(np.abs(s))))


@pytest.mark.parametrize("Lv,K,alpha,bits", [(5, 2, 2, 31), (3, 2, 2, 31), (3, 1, 1, 31), (3, 3, 3, 31), (3, 2, 2, 61)])
def test_keyswitch_products_and_decryption_bound(Lv, K, alpha, bits):
    """The sums use exact negacyclic products (orc.mul_naive gives the same
    words) and acc0 + acc1 s - x s' stays within
    N sum_d |I_d| Q_d max|e_d| / P + (K + 1)(1 + |s|_1), at the full level and,
    with restrict_key, one level down."""
    mod = _moduli(Lv, K, bits)
    rng = np.random.default_rng(10 * Lv + alpha)
    Be = orc.Basis(mod, N)
    s, sp = _ternary(rng, N, N // 2), _ternary(rng, N, N // 2)
    key_a, key_b, emax = _hybrid_keys(Be, mod, Lv, alpha, s, sp, rng)
    for lv in (Lv, Lv - 1):
        modl = mod[:lv] + mod[Lv:]
        Bel, Bc = orc.Basis(modl, N), orc.Basis(mod[:lv], N)
        ka, kb = restrict_key(key_a, Lv, alpha, lv), restrict_key(key_b, Lv, alpha, lv)
        assert ka.shape == (n_digits(lv, alpha), lv + K, N)
        x = orc.uniform_poly(mod[:lv], N, rng)
        acc0, acc1 = keyswitch_hybrid_ref(Bel, lv, x, ka, kb, alpha)
        n0, n1 = keyswitch_hybrid_ref(Bel, lv, x, ka, kb, alpha, mul=lambda u, v: orc.mul_naive(Bel, u, v))
        assert np.array_equal(acc0, n0) and np.array_equal(acc1, n1)
        q = np.array(mod[:lv], dtype=np.uint64)[:, None]
        assert (acc0 < q).all() and (acc1 < q).all()
        err = _decrypt_error(Bc, mod[:lv], acc0, acc1, x, s, sp)
        bound = _bound(modl, lv, K, alpha, emax, s)
        # the one-limb gadget on the same ring, for comparison
        ga = orc.uniform_poly(mod[:lv], N, rng, batch=lv)
        gb = np.zeros_like(ga)
        sC, spC = lift_small(s, mod[:lv]), lift_small(sp, mod[:lv])
        for i in range(lv):
            e = lift_small(np.rint(rng.normal(0, 3.2, N)).astype(np.int64), mod[:lv])
            gb[i] = orc.add(Bc, orc.neg(Bc, orc.mul(Bc, ga[i], sC)), e)
            gb[i, i] = (gb[i, i] + spC[i]) % np.uint64(mod[i])
        g0, g1 = orc.keyswitch(Bc, x, ga, gb)
        gerr = _decrypt_error(Bc, mod[:lv], g0, g1, x, s, sp)
        print(f"Lv={lv} K={K} alpha={alpha} bits={bits}: hybrid error {err} (2^{_log2(err):.1f}), "
              f"bound {bound}; gadget error 2^{_log2(gerr):.1f}")
        assert err <= bound, (lv, err, bound)
