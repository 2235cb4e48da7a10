"""rnt_mul_monomial on the GPU, exact against numpy (tests/homdft_ref.py
mul_monomial_ref: the definition of the negacyclic shift).  The inputs hold
zeros and q - 1 words next to uniform ones, so that the negation of 0 (which
stays 0) and of the largest residue are seen."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
from homdft_ref import mul_monomial_ref
from test_gpu_unaligned import guards, shifted

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, DOMAIN = 11, 7
L = 3


def shifts(n):
    return [0, 1, n - 1, n, n + 1, 2 * n - 1, n // 2, 3 * n // 2, -1, -n // 2, 2 * n, (1 << 40) + 3]


def make_input(mod, n, B, rng):
    x = orc.uniform_poly(mod, n, rng, batch=B)
    q = np.array(mod, dtype=np.uint64)[:, None]
    x[0, :, ::5] = 0
    x[0, :, 1::7] = np.broadcast_to(q - np.uint64(1), (len(mod), n))[:, 1::7]
    x[B - 1, :, :4] = 0
    x[B - 1, :, n - 4:] = np.broadcast_to(q - np.uint64(1), (len(mod), 4))
    return x


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("bits", [31, 61])
@pytest.mark.parametrize("log_n", [8, 12, 14])
def test_mul_monomial_matches_numpy(gpu, log_n, bits, B):
    rn = gpu
    n = 1 << log_n
    mod = orc.generate_primes(bits, L, n)
    basis = rn.RnsBasis(mod, n)
    x = make_input(mod, n, B, np.random.default_rng(log_n * 100 + bits + B))
    src = rn.RnsPoly.from_channels(x, basis)
    basis.profile_enable(True)
    try:
        for k in shifts(n):
            out = src.mul_monomial(k)
            assert not out.is_ntt_domain()
            assert np.array_equal(out.channels_batch(), mul_monomial_ref(x, mod, k)), f"k = {k}"
            # X^k then X^(2N - k) is the identity
            assert np.array_equal(out.mul_monomial(2 * n - k).channels_batch(), x), f"k = {k}: the way back"
        assert basis.profile_read("mul_monomial")[0] == 2 * len(shifts(n))
    finally:
        basis.profile_enable(False)
    assert np.array_equal(src.channels_batch(), x)


@pytest.mark.parametrize("bits", [31, 61])
def test_mul_monomial_on_a_drop_last_view_and_word_aligned_buffers(gpu, bits):
    rn = gpu
    n, B = 4096, 3
    mod = orc.generate_primes(bits, L, n)
    root = rn.RnsBasis(mod, n)
    view = root.drop_last(1)
    x = make_input(mod[:L - 1], n, B, np.random.default_rng(bits))
    src = rn.RnsPoly.from_channels(x, view)
    for k in (n // 2, 3 * n // 2, 5, -7):
        assert np.array_equal(src.mul_monomial(k).channels_batch(), mul_monomial_ref(x, mod[:L - 1], k))
    # one word past a 16-byte boundary on both sides, between guard words
    s = shifted(rn, view, x)
    for k in (n // 2, 4, 3, 2 * n - 1):  # (4: a whole vector's shift; 3: not one)
        o = shifted(rn, view, B)
        rn.check(rn.load().rnt_mul_monomial(o.handle, s.handle, k))
        assert np.array_equal(o.channels_batch(), mul_monomial_ref(x, mod[:L - 1], k))
        guards(s, o)
    # an aligned output from a word-aligned input
    o = rn.RnsPoly(view, B)
    rn.check(rn.load().rnt_mul_monomial(o.handle, s.handle, n + 1))
    assert np.array_equal(o.channels_batch(), mul_monomial_ref(x, mod[:L - 1], n + 1))
    guards(s)


def test_mul_monomial_refusals(gpu):
    rn = gpu
    lib = rn.load()
    n, B = 256, 2
    mod = orc.generate_primes(31, L, n)
    basis = rn.RnsBasis(mod, n)
    x = make_input(mod, n, B, np.random.default_rng(3))
    src = rn.RnsPoly.from_channels(x, basis)
    assert lib.rnt_mul_monomial(src.handle, src.handle, 1) == BAD_ARGUMENT  # out == in
    assert np.array_equal(src.channels_batch(), x)
    out = rn.RnsPoly.from_channels(x, basis)
    ntt = rn.RnsPoly.from_channels(x, basis, in_ntt_domain=True)
    assert lib.rnt_mul_monomial(out.handle, ntt.handle, 1) == DOMAIN
    assert np.array_equal(out.channels_batch(), x) and not out.is_ntt_domain()
