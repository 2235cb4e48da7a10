"""The two identities the fused hybrid multiply + rescale rests on, and the
yardstick itself, on the CPU at N = 32:

  * ModDown(A + lift(P d)) = ModDown(A) + d mod q, word for word -- the seeds
    of the multiply may enter the accumulator before ModDown;
  * the per-coefficient formula of k_moddown_rescale is rescale(ModDown(A) +
    add), also on all-(m - 1) inputs.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from hybrid_ref import moddown_ref, mul_relin_hybrid_ref, n_digits
from hybrid_rescale_ref import (add_over, lift_P_times, moddown_rescale_fused, mul_relin_rescale_hybrid_ref)

N = 32


def _primes(bits, count):
    out, c = [], (1 << (bits - 1)) + 1
    while len(out) < count:
        if _is_prime(c):  # c = 1 mod 2N: NTT-friendly
            out.append(c)
        c += 2 * N
    return out


def _is_prime(c):
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if c % a == 0:
            return c == a
    d, s = c - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        x = pow(a, d, c)
        if x in (1, c - 1):
            continue
        for _ in range(s - 1):
            x = x * x % c
            if x == c - 1:
                break
        else:
            return False
    return True


@pytest.fixture(scope="module", params=[(31, 3, 2), (31, 2, 1), (61, 3, 2)], ids=lambda p: "bits%d-Lv%d-K%d" % p)
def ring(request):
    bits, Lv, K = request.param
    return _primes(bits, Lv + K), Lv, K


@pytest.mark.parametrize("seed", range(4))
def test_moddown_of_a_seeded_accumulator(ring, seed):
    emod, Lv, K = ring
    rng = np.random.default_rng(9100 + seed)
    A = orc.uniform_poly(emod, N, rng)
    d = orc.uniform_poly(emod[:Lv], N, rng)
    lift = lift_P_times(emod, Lv, d)
    assert not lift[Lv:].any()  # P d vanishes on the special limbs
    got = moddown_ref(emod, Lv, add_over(emod, A, lift))
    want = add_over(emod[:Lv], moddown_ref(emod, Lv, A), d)
    assert np.array_equal(got, want)


def _edge(emod, Lv):
    mm1 = np.array([m - 1 for m in emod], dtype=np.uint64)[:, None]
    return np.ascontiguousarray(np.broadcast_to(mm1, (len(emod), N))), np.ascontiguousarray(
        np.broadcast_to(mm1[:Lv], (Lv, N)))


@pytest.mark.parametrize("with_add", [False, True])
def test_fused_formula_is_rescale_of_moddown(ring, with_add):
    emod, Lv, K = ring
    Bc = orc.Basis(emod[:Lv], N)
    rng = np.random.default_rng(9200 + Lv + K)
    cases = [(orc.uniform_poly(emod, N, rng), orc.uniform_poly(emod[:Lv], N, rng)) for _ in range(3)]
    cases.append(_edge(emod, Lv))
    zero = np.zeros((Lv + K, N), dtype=np.uint64)
    cases.append((zero, _edge(emod, Lv)[1]))
    for A, add in cases:
        r = moddown_ref(emod, Lv, A)
        if with_add:
            r = add_over(emod[:Lv], r, add)
        want = orc.rescale(Bc, r)
        got = moddown_rescale_fused(emod, Lv, A, add if with_add else None)
        assert got.shape == (Lv - 1, N)
        assert np.array_equal(got, want)


def test_yardstick_is_the_composition():
    emod, Lv, K, alpha = _primes(31, 5), 3, 2, 2
    mod = emod[:Lv]
    Bc, Be = orc.Basis(mod, N), orc.Basis(emod, N)
    rng = np.random.default_rng(9300)
    c = [orc.uniform_poly(mod, N, rng) for _ in range(4)]
    beta = n_digits(Lv, alpha)
    ka, kb = orc.uniform_poly(emod, N, rng, batch=beta), orc.uniform_poly(emod, N, rng, batch=beta)
    r0, r1 = mul_relin_hybrid_ref(Bc, Be, *c, ka, kb, alpha)
    g0, g1 = mul_relin_rescale_hybrid_ref(Bc, Be, *c, ka, kb, alpha)
    assert g0.shape == (Lv - 1, N)
    assert np.array_equal(g0, orc.rescale(Bc, r0)) and np.array_equal(g1, orc.rescale(Bc, r1))
    # and it is the fused formula on the key-switch accumulators with the seeds as addends
    from hybrid_ref import modup_ref

    d0 = orc.mul(Bc, c[0], c[2])
    d2 = orc.mul(Bc, c[1], c[3])
    A0 = None
    for d in range(beta):
        p = orc.mul(Be, modup_ref(emod, Lv, alpha, d, d2), kb[d])
        A0 = p if A0 is None else orc.add(Be, A0, p)
    assert np.array_equal(moddown_rescale_fused(emod, Lv, A0, d0), g0)
    seeded = add_over(emod, A0, lift_P_times(emod, Lv, d0))
    assert np.array_equal(moddown_rescale_fused(emod, Lv, seeded), g0)
