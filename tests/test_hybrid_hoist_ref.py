"""The yardstick of the hoisted hybrid rotation and of the hybrid baby-step
giant-step transform (tests/hybrid_hoist_ref.py) on the CPU, at N = 32: the
hoisting form, why sigma stands outside ModDown, the decryption and its error
against the bound that follows from the definition, the restriction to a lower
level -- pinned here before any GPU run relies on it."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
import test_hybrid_ref as thr
from hoist_ref import rotation_exponent
from hybrid_hoist_ref import (bsgs_hybrid_ref, hoisted_sums, hybrid_hoisting_form_coeff, rotate_hybrid_hoisted_ref)
from hybrid_ref import crt_centered, lift_small, moddown_ref, n_digits, restrict_key, rotate_hybrid_ref

N = thr.N
RINGS = [(3, 2, 2, 31), (3, 1, 1, 31), (3, 3, 3, 31), (3, 2, 2, 61)]  # (Lv, K, alpha, bits)


def _sigma_int(v, k):
    """rotate_slots(., k) of a polynomial with Python-int coefficients."""
    g = rotation_exponent(k, N)
    out = [0] * N
    for i, c in enumerate(v):
        t = i * g % (2 * N)
        out[t % N] = -int(c) if t >= N else int(c)
    return out


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_hoisted_form_is_the_inverse_automorphism_of_the_key(Lv, K, alpha, bits):
    """The definition with sigma_k^-1(key) spelt as orc.automorphism by g^-1 on
    the coefficient-domain key, step by step, gives rotate_hybrid_hoisted_ref's
    words; and those are not rotate_hybrid_ref's."""
    mod = thr._moduli(Lv, K, bits)
    Bc, Be = orc.Basis(mod[:Lv], N), orc.Basis(mod, N)
    rng = np.random.default_rng(300 + Lv + K)
    beta = n_digits(Lv, alpha)
    c0, c1 = orc.uniform_poly(mod[:Lv], N, rng), orc.uniform_poly(mod[:Lv], N, rng)
    ka, kb = orc.uniform_poly(mod, N, rng, batch=beta), orc.uniform_poly(mod, N, rng, batch=beta)
    for k in (1, -3, 5):
        g = rotation_exponent(k, N)
        ginv = pow(g, -1, 2 * N)
        assert g * ginv % (2 * N) == 1
        ha = np.stack([orc.automorphism(Be, ka[d], ginv)[0] for d in range(beta)])
        hb = np.stack([orc.automorphism(Be, kb[d], ginv)[0] for d in range(beta)])
        assert np.array_equal(ha, hybrid_hoisting_form_coeff(Be, ka, k))
        for d in range(beta):  # sigma_k of the hoisting form is the key again
            assert np.array_equal(orc.automorphism(Be, ha[d], g)[0], ka[d])
        A0, A1 = hoisted_sums(Be, Lv, c1, ha, hb, alpha)
        w0 = orc.automorphism(Bc, orc.add(Bc, c0, moddown_ref(mod, Lv, A0)), g)[0]
        w1 = orc.automorphism(Bc, moddown_ref(mod, Lv, A1), g)[0]
        r0, r1 = rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, k, ka, kb, alpha)
        assert np.array_equal(r0, w0) and np.array_equal(r1, w1)
        n0, n1 = rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, k, ka, kb, alpha, mul=lambda u, v: orc.mul_naive(Be, u, v))
        assert np.array_equal(r0, n0) and np.array_equal(r1, n1)
        o0, o1 = rotate_hybrid_ref(Bc, Be, c0, c1, k, ka, kb, alpha)
        assert not np.array_equal(r0, o0) and not np.array_equal(r1, o1)
    z0, z1 = rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, 0, None, None, alpha)
    assert np.array_equal(z0, c0) and np.array_equal(z1, c1)


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_sigma_does_not_commute_with_moddown(Lv, K, alpha, bits):
    mod = thr._moduli(Lv, K, bits)
    Bc, Be = orc.Basis(mod[:Lv], N), orc.Basis(mod, N)
    A = orc.uniform_poly(mod, N, np.random.default_rng(310))
    outside = orc.rotate_slots(Bc, moddown_ref(mod, Lv, A), 1)[0]
    inside = moddown_ref(mod, Lv, orc.rotate_slots(Be, A, 1)[0])
    assert not np.array_equal(outside, inside)
    # ... though they differ by the quotient's few units only: both are valid
    d = crt_centered(orc.add(Bc, outside, orc.neg(Bc, inside)), mod[:Lv])
    assert 0 < max(abs(v) for v in d) <= K


def _setup(Lv, K, alpha, bits, seed):
    mod = thr._moduli(Lv, K, bits)
    Bc, Be = orc.Basis(mod[:Lv], N), orc.Basis(mod, N)
    rng = np.random.default_rng(seed)
    s = thr._ternary(rng, N, N // 2)
    return mod, Bc, Be, rng, s


def _rot_key(Be, mod, Lv, alpha, s, k, rng):
    """The hybrid rotation key of step k: target sigma_k(s)."""
    return thr._hybrid_keys(Be, mod, Lv, alpha, s, np.array(_sigma_int(s, k), dtype=np.int64), rng)


def _encrypt(Bc, modc, s, m, rng):
    c1 = orc.uniform_poly(modc, N, rng)
    e = np.rint(rng.normal(0, 3.2, N)).astype(np.int64)
    c0 = orc.add(Bc, orc.neg(Bc, orc.mul(Bc, c1, lift_small(s, modc))), lift_small(m + e, modc))
    return c0, c1, m + e


def _decrypt(Bc, modc, c0, c1, s):
    return crt_centered(orc.add(Bc, c0, orc.mul(Bc, c1, lift_small(s, modc))), modc)


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_hoisted_rotation_decrypts_to_the_rotated_message(Lv, K, alpha, bits):
    """c0 + c1 s = m  ->  out0 + out1 s = sigma_k(m) + error, the error within
    the key-switch bound of tests/test_hybrid_ref.py (sigma preserves norms, and
    the inner pair is a key-switch from s to sigma_k^-1(s) under the key
    sigma_k^-1(key), whose errors are the key's permuted)."""
    mod, Bc, Be, rng, s = _setup(Lv, K, alpha, bits, 320 + Lv + K)
    m = rng.integers(-(1 << 20), 1 << 20, N)
    c0, c1, me = _encrypt(Bc, mod[:Lv], s, m, rng)
    for k in (1, -3):
        ka, kb, emax = _rot_key(Be, mod, Lv, alpha, s, k, rng)
        o0, o1 = rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, k, ka, kb, alpha)
        got = _decrypt(Bc, mod[:Lv], o0, o1, s)
        want = _sigma_int(me, k)
        err = max(abs(a - b) for a, b in zip(got, want))
        bound = thr._bound(mod, Lv, K, alpha, emax, s)
        print(f"Lv={Lv} K={K} alpha={alpha} bits={bits} k={k}: error {err}, bound {bound}")
        assert err <= bound


@pytest.mark.parametrize("seed", [330, 331, 332, 333])
def test_bsgs_decrypts_to_the_matrix_vector_sum_and_is_no_noisier_than_the_composition(seed):
    """out0 + out1 s = sum_j sigma_{g_j}(sum_i p_ji sigma_{b_i}(m)) + error, and
    that error does not exceed the error of the composition of rotate_hybrid_ref
    calls on the same draws plus (K + 1)(1 + |s|_1).

    The composition here runs its giant stage -- rotate_hybrid_ref per nonzero
    giant, orc.add -- on the SAME R_i as the transform (the hoisted baby
    rotations).  With the baby rotations taken from rotate_hybrid_ref as well
    the comparison is not a theorem and fails draw by draw (seed 330: transform
    2604, that composition 2054, the term 51): the two baby stages round
    differently (ModUp sees c1 in one, sigma(c1) in the other) and the plaintext
    products multiply that difference by |p|_1.  On the same R_i the V_j agree
    and the two differ in the giant stage alone, where the definition fixes the
    difference: ModDown(A) = (A - c(A)) / P with c(A) = [A]_P + v P, 0 <= v < K,
    so for n = |NZ| giants, per coefficient and component,

        ModDown(sum_j A_j) - sum_j ModDown(A_j) = sum_j v_j + w - v  in [-(K - 1), n K - 1]

    (w in [0, n - 1] the carries of sum_j [A_j]_P).  The test asserts that range
    word for word -- it is what 'one ModDown for all giants' means, and a
    transform that divided once per giant would give 0 everywhere -- and from
    it error <= composition's error + (n K - 1)(1 + |s|_1), which for this
    case's n = 2, K = 2 is the (K + 1)(1 + |s|_1) of one ModDown.  The bound
    derived from the draws as tests/test_hybrid_ref.py derives its own (the
    ModDown term once instead of once per giant) is asserted too."""
    Lv, K, alpha, bits = 3, 2, 2, 31
    mod, Bc, Be, rng, s = _setup(Lv, K, alpha, bits, seed)
    modc = mod[:Lv]
    baby, giant = [0, 1, -3], [4, 0, -8, 0]
    n1 = len(baby)
    m = rng.integers(-(1 << 12), 1 << 12, N)
    c0, c1, me = _encrypt(Bc, modc, s, m, rng)
    bk3 = [None if b == 0 else _rot_key(Be, mod, Lv, alpha, s, b, rng) for b in baby]
    gk3 = [None if g == 0 else _rot_key(Be, mod, Lv, alpha, s, g, rng) for g in giant]
    bk = [None if k is None else k[:2] for k in bk3]
    gk = [None if k is None else k[:2] for k in gk3]
    pl = [rng.integers(-8, 9, N) for _ in range(n1 * len(giant))]  # small plaintext polys
    diag = [lift_small(p, modc) for p in pl]
    o0, o1 = bsgs_hybrid_ref(Bc, Be, c0, c1, baby, giant, diag, bk, gk, alpha)
    got = _decrypt(Bc, modc, o0, o1, s)

    def negacyclic(a, b):
        out = [0] * N
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                t = i + j
                out[t % N] += -int(x) * int(y) if t >= N else int(x) * int(y)
        return out

    want = [0] * N
    for j, g in enumerate(giant):
        v = [0] * N
        for i, b in enumerate(baby):
            r = _sigma_int(me, b) if b else [int(x) for x in me]
            v = [x + y for x, y in zip(v, negacyclic(pl[j * n1 + i], r))]
        v = _sigma_int(v, g) if g else v
        want = [x + y for x, y in zip(want, v)]
    err = max(abs(a - b) for a, b in zip(got, want))

    def compose(rot):
        """The giant stage as rotate_hybrid_ref calls and adds on the R_i `rot`."""
        t0 = t1 = None
        for j, g in enumerate(giant):
            v0 = v1 = None
            for i in range(n1):
                p0, p1 = orc.mul(Bc, rot[i][0], diag[j * n1 + i]), orc.mul(Bc, rot[i][1], diag[j * n1 + i])
                v0 = p0 if v0 is None else orc.add(Bc, v0, p0)
                v1 = p1 if v1 is None else orc.add(Bc, v1, p1)
            r0, r1 = rotate_hybrid_ref(Bc, Be, v0, v1, g, *(gk[j] or (None, None)), alpha)
            t0 = r0 if t0 is None else orc.add(Bc, t0, r0)
            t1 = r1 if t1 is None else orc.add(Bc, t1, r1)
        return t0, t1

    hoisted = [rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, b, *(bk[i] or (None, None)), alpha) for i, b in enumerate(baby)]
    t0, t1 = compose(hoisted)
    nz = [k3 for k3 in gk3 if k3 is not None]
    n = len(nz)
    assert n == 2 and n * K - 1 == K + 1
    # the words: the transform minus the composition is the ModDowns' difference
    seen = set()
    for o, t in ((o0, t0), (o1, t1)):
        d = crt_centered(orc.add(Bc, o, orc.neg(Bc, t)), modc)
        assert all(-(K - 1) <= v <= n * K - 1 for v in d), (min(d), max(d))
        seen |= set(d)
    assert seen != {0}  # not the composition's words: one ModDown, not one per giant
    err_c = max(abs(a - b) for a, b in zip(_decrypt(Bc, modc, t0, t1, s), want))
    term = (K + 1) * (1 + int(np.sum(np.abs(s))))
    # for the record: the composition with rotate_hybrid_ref's baby rotations too
    l0, l1 = compose([rotate_hybrid_ref(Bc, Be, c0, c1, b, *(bk[i] or (None, None)), alpha) for i, b in enumerate(baby)])
    err_l = max(abs(a - b) for a, b in zip(_decrypt(Bc, modc, l0, l1, s), want))
    bound_c = 0
    for j in range(len(giant)):
        for i, k3 in enumerate(bk3):
            if k3 is not None:
                bound_c += int(np.sum(np.abs(pl[j * n1 + i]))) * thr._bound(mod, Lv, K, alpha, k3[2], s)
    bound_c += sum(thr._bound(mod, Lv, K, alpha, k3[2], s) for k3 in nz)
    bound = bound_c - (n - 1) * term
    print(f"seed {seed}: bsgs error {err}, composition on the same R_i {err_c} (+ term {term}), differences seen "
          f"{sorted(seen)}; composition with rotate_hybrid_ref babies {err_l}; bounds {bound} / {bound_c}")
    assert err <= err_c + term
    assert err_c <= bound_c and err <= bound


@pytest.mark.parametrize("k", [1, -3])
def test_restriction_commutes_with_the_hoisting_form(k):
    Lv, K, alpha = 4, 2, 2
    mod = thr._moduli(Lv, K, 31)
    Be = orc.Basis(mod, N)
    low = mod[:3] + mod[Lv:]
    Bl = orc.Basis(low, N)
    key = orc.uniform_poly(mod, N, np.random.default_rng(340), batch=n_digits(Lv, alpha))
    a = restrict_key(hybrid_hoisting_form_coeff(Be, key, k), Lv, alpha, 3)
    b = hybrid_hoisting_form_coeff(Bl, restrict_key(key, Lv, alpha, 3), k)
    assert np.array_equal(a, b)
    # and in the NTT domain, the form the device keeps
    keep = [0, 1, 2, 4, 5]
    full_ntt = np.stack([orc.to_ntt(Be, p) for p in hybrid_hoisting_form_coeff(Be, key, k)])
    low_ntt = np.stack([orc.to_ntt(Bl, p) for p in b])
    assert np.array_equal(full_ntt[: n_digits(3, alpha)][:, keep, :], low_ntt)
