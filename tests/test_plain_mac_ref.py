"""The CPU model of the plaintext multiply-accumulate (tests/plain_mac_ref.py)
against schoolbook negacyclic products in Python integers: shared and
per-ciphertext plaintexts, with and without bias, plain and rescaled."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from plain_mac_ref import pick_plain, pick_terms, plain_mac_ref


def _schoolbook(a, b, q):
    """a b mod (X^N + 1, q) on Python integers."""
    n = len(a)
    out = [0] * n
    for i, ai in enumerate(a):
        ai = int(ai)
        for j, bj in enumerate(b):
            k = i + j
            if k < n:
                out[k] += ai * int(bj)
            else:
                out[k - n] -= ai * int(bj)
    return [v % q for v in out]


def _rescale_int(r, mod):
    """poly.rs rescale on Python integers: (c_t - (c_last mod q_t)) q_last^-1 mod q_t."""
    ql = mod[-1]
    out = []
    for t, q in enumerate(mod[:-1]):
        inv = pow(ql % q, -1, q)
        out.append([((int(c) - int(cl) % q) * inv) % q for c, cl in zip(r[t], r[-1])])
    return np.array(out, dtype=np.uint64)


@pytest.mark.parametrize("log_n", [4, 6])
@pytest.mark.parametrize("bits", [31, 61])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("biased", [False, True])
def test_model_is_the_schoolbook_sum(log_n, bits, shared, biased):
    n, Lv, B, n_terms = 1 << log_n, 3, 2, 3
    mod = orc.generate_primes(bits, Lv, n)
    Bo = orc.Basis(mod, n)
    rng = np.random.default_rng(1000 * log_n + bits + 2 * shared + biased)
    x0 = orc.uniform_poly(mod, n, rng, batch=n_terms * B)
    x1 = orc.uniform_poly(mod, n, rng, batch=n_terms * B)
    m_coeff = orc.uniform_poly(mod, n, rng, batch=n_terms if shared else n_terms * B)
    b_coeff = orc.uniform_poly(mod, n, rng, batch=B)
    m_ntt = np.stack([orc.to_ntt(Bo, p) for p in m_coeff])
    b_ntt = np.stack([orc.to_ntt(Bo, p) for p in b_coeff])
    for p in range(B):
        t0, t1 = pick_terms(x0, p, B), pick_terms(x1, p, B)
        mc = pick_plain(m_coeff, p, B, n_terms)
        want = []
        for comp, add in ((t0, b_coeff[p] if biased else None), (t1, None)):
            rows = []
            for t, q in enumerate(mod):
                acc = [0] * n
                for i in range(n_terms):
                    acc = [(u + v) % q for u, v in zip(acc, _schoolbook(comp[i][t], mc[i][t], q))]
                if add is not None:
                    acc = [(u + int(v)) % q for u, v in zip(acc, add[t])]
                rows.append(acc)
            want.append(np.array(rows, dtype=np.uint64))
        args = (Bo, t0, t1, pick_plain(m_ntt, p, B, n_terms), b_ntt[p] if biased else None)
        got = plain_mac_ref(*args)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        got = plain_mac_ref(*args, rescale=True)
        assert got[0].shape == (Lv - 1, n)
        assert np.array_equal(got[0], _rescale_int(want[0], mod))
        assert np.array_equal(got[1], _rescale_int(want[1], mod))


def test_one_term_is_the_product():
    n, Lv = 64, 2
    mod = orc.generate_primes(31, Lv, n)
    Bo = orc.Basis(mod, n)
    rng = np.random.default_rng(5)
    c0, c1, m = (orc.uniform_poly(mod, n, rng) for _ in range(3))
    r0, r1 = plain_mac_ref(Bo, c0[None], c1[None], orc.to_ntt(Bo, m)[None])
    assert np.array_equal(r0, orc.mul(Bo, c0, m)) and np.array_equal(r1, orc.mul(Bo, c1, m))
