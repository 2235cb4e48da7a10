"""The matrix-core kernels (k_mf_mul, k_mf_ntt, k_mf_tensor) with the
quotient-estimate reduction (recomb_q, RNT_MF_QR) in their passes, at the
smallest shape they run at: N = 2^16, L = 2, batch 2, on two bases: the first
two metric primes and the two ends of the 31-bit range.

Full outputs, word for word: rnt_mul against the oracle (uniform, all q-1,
zero and monomial operands, also with the result aliasing either operand);
the standalone transforms against the oracle and their round trip; the
ciphertext tensor against the four-step kernels (RNT_PLANE=0).  A wrong
broadcast of the MFMA's inline-constant accumulator (the reduction's rounding
offset) would put words outside the packed range and fail every one of these.
A basis with a 30-bit prime either runs bit-exactly or is refused by name.
"""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc

pytestmark = pytest.mark.gpu

N, L, B = 1 << 16, 2, 2
MONOMIALS = (1, 15, 16, 255, 256, 4095, 4096, 65535)
ENDS = [1073872897, 2147352577]  # the smallest and the largest NTT-friendly 31-bit prime


def _moduli(rn, name):
    return rn.generate_primes(31, 16, N)[:L] if name == "metric" else list(ENDS)


@pytest.fixture(scope="module", params=["metric", "ends"])
def ring(request, gpu):
    rn = gpu
    mod = _moduli(rn, request.param)
    Bo = orc.Basis(mod, N)
    rng = np.random.default_rng(0x0B0E)
    a_h = orc.uniform_poly(mod, N, rng, batch=B)
    b_h = orc.uniform_poly(mod, N, rng, batch=B)
    q = np.array(mod, dtype=np.uint64)[:, None]
    top = np.broadcast_to(q - 1, (B, L, N)).copy()
    zero = np.zeros((B, L, N), dtype=np.uint64)
    cases = {"uniform": (a_h, b_h), "top": (top, top), "zero": (zero, b_h)}
    want = {k: [orc.mul(Bo, x[i], y[i]) for i in range(B)] for k, (x, y) in cases.items()}
    return rn, mod, Bo, rn.RnsBasis(mod, N), cases, want


def _check(got, want, what):
    for i in range(B):
        assert np.array_equal(got[i], want[i]), (what, i)


def _monomial(b_h, q, j):
    a_h = np.zeros((B, L, N), dtype=np.uint64)
    a_h[:, :, j] = 1
    want = np.empty_like(b_h)
    want[:, :, j:] = b_h[:, :, : N - j]
    want[:, :, :j] = (q - b_h[:, :, N - j :]) % q
    return a_h, want


@pytest.mark.parametrize("case", ["uniform", "top", "zero"])
def test_mul_full_output_and_aliased(ring, case):
    rn, mod, Bo, Bd, cases, want = ring
    a_h, b_h = cases[case]
    c = rn.RnsPoly.from_channels(a_h, Bd) * rn.RnsPoly.from_channels(b_h, Bd)
    _check(c.channels(), want[case], case)
    a, b = rn.RnsPoly.from_channels(a_h, Bd), rn.RnsPoly.from_channels(b_h, Bd)
    a *= b  # c aliases a
    _check(a.channels(), want[case], (case, "c = a"))
    assert np.array_equal(b.channels(), b_h)
    a = rn.RnsPoly.from_channels(a_h, Bd)
    rn.check(rn.load().rnt_mul(b.handle, a.handle, b.handle))  # c aliases b
    _check(b.channels(), want[case], (case, "c = b"))
    assert np.array_equal(a.channels(), a_h)


def test_mul_monomials(ring):
    """a = X^j: the product is b shifted by j with the wrapped words negated
    (computed without the oracle's transform, compared with it once)."""
    rn, mod, Bo, Bd, cases, _ = ring
    b_h = cases["uniform"][1]
    q = np.array(mod, dtype=np.uint64)[:, None]
    b = rn.RnsPoly.from_channels(b_h, Bd)
    for j in MONOMIALS:
        a_h, want = _monomial(b_h, q, j)
        if j == MONOMIALS[0]:
            assert np.array_equal(want[0], orc.mul(Bo, a_h[0], b_h[0]))
        c = rn.RnsPoly.from_channels(a_h, Bd) * b
        assert np.array_equal(c.channels(), want), j


def test_mul_monomials_aliased(ring):
    rn, mod, Bo, Bd, cases, _ = ring
    b_h = cases["uniform"][1]
    q = np.array(mod, dtype=np.uint64)[:, None]
    for j in MONOMIALS:
        a_h, want = _monomial(b_h, q, j)
        a, b = rn.RnsPoly.from_channels(a_h, Bd), rn.RnsPoly.from_channels(b_h, Bd)
        a *= b
        assert np.array_equal(a.channels(), want), (j, "c = a")
        a = rn.RnsPoly.from_channels(a_h, Bd)
        rn.check(rn.load().rnt_mul(b.handle, a.handle, b.handle))
        assert np.array_equal(b.channels(), want), (j, "c = b")


def test_transforms_full_output_and_round_trip(ring):
    rn, mod, Bo, Bd, cases, _ = ring
    for name in ("uniform", "top"):
        a_h = cases[name][0]
        t = rn.RnsPoly.from_channels(a_h, Bd)
        t.to_ntt_domain()
        assert t.is_ntt_domain()
        nt = [orc.to_ntt(Bo, a_h[i]) for i in range(B)]
        _check(t.channels(), nt, name)
        t.to_coeff_domain()
        assert not t.is_ntt_domain()
        assert np.array_equal(t.channels(), a_h), name


def test_tensor_full_output_against_four_step(ring, monkeypatch):
    rn, mod, Bo, Bd, cases, want = ring
    a_h, b_h = cases["uniform"]
    c = [a_h[:1], b_h[:1], b_h[1:], a_h[1:]]  # one ciphertext pair
    outs = {}
    for plane in (None, "0"):
        if plane is None:
            monkeypatch.delenv("RNT_PLANE", raising=False)
        else:
            monkeypatch.setenv("RNT_PLANE", plane)
        bd = rn.RnsBasis(mod, N)
        d = rn.ct_tensor(*(rn.RnsPoly.from_channels(np.ascontiguousarray(x), bd) for x in c))
        outs[plane] = [x.channels() for x in d]
    for i in range(3):
        assert np.array_equal(outs[None][i], outs["0"][i]), i
    assert np.array_equal(outs[None][2][0], orc.mul(Bo, c[1][0], c[3][0]))


def test_30_bit_prime_exact_or_refused(gpu):
    """The reduction's margins shrink with q: a basis with a 30-bit prime
    runs bit-exactly or rnt_ctx_create refuses it with mf_build's message."""
    rn = gpu
    mod = [rn.generate_primes(30, 1, N)[0], rn.generate_primes(31, 1, N)[0]]
    try:
        Bd = rn.RnsBasis(mod, N)
    except rn.RnsNttError as e:
        assert "MFMA tables" in str(e), str(e)
        return
    Bo = orc.Basis(mod, N)
    rng = np.random.default_rng(0x30B)
    a_h = orc.uniform_poly(mod, N, rng, batch=B)
    q = np.array(mod, dtype=np.uint64)[:, None]
    top = np.broadcast_to(q - 1, (B, L, N)).copy()
    for x, y, what in ((a_h, top, "uniform x top"), (top, top, "top x top")):
        c = rn.RnsPoly.from_channels(x, Bd) * rn.RnsPoly.from_channels(y, Bd)
        _check(c.channels(), [orc.mul(Bo, x[i], y[i]) for i in range(B)], what)
    t = rn.RnsPoly.from_channels(a_h, Bd)
    t.to_ntt_domain()
    _check(t.channels(), [orc.to_ntt(Bo, a_h[i]) for i in range(B)], "ntt")
    t.to_coeff_domain()
    assert np.array_equal(t.channels(), a_h)
