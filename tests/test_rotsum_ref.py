"""The yardstick of the rotate-and-sum (tests/rotsum_ref.py) on the CPU, at
N = 32: the decryption with a noise-free key, the single-step and all-zero
cases, and the index function of the automorphism in the NTT domain -- a
bijection, block-structured, and the oracle's own sigma_g -- pinned here before
any GPU run relies on it."""
from __future__ import annotations

import numpy as np
import pytest

import pyoracle as orc
import test_hybrid_hoist_ref as thh
import test_hybrid_ref as thr
from hoist_ref import rotation_exponent
from hybrid_ref import crt_centered, hybrid_key_plain, lift_small, rotate_hybrid_ref
from rotsum_ref import ntt_automorphism_source, rotsum_hybrid_ref

N = thr.N
RINGS = [(3, 2, 2, 31), (3, 1, 1, 31), (3, 3, 3, 31), (3, 2, 2, 61)]  # (Lv, K, alpha, bits)
STEPS = [0, 1, -3, 0, 5, 1]


def _plain_key(mod, Lv, alpha, s, k):
    """The noise-free hybrid rotation key of step k: key_a = 0, key_b = the
    plaintexts G_d of the target sigma_k(s)."""
    target = lift_small(np.array(thh._sigma_int(s, k), dtype=np.int64), mod[:Lv])
    kb = hybrid_key_plain(mod, Lv, alpha, target)
    return np.zeros_like(kb), kb


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_noise_free_key_decrypts_to_the_sum_of_rotations(Lv, K, alpha, bits):
    """c0 + c1 s = m  ->  out0 + out1 s = z m + sum_{t in NZ} sigma_{k_t}(m) +
    error with |error| <= (K + 1)(1 + |s|_1), the ModDown bound of
    tests/test_hybrid_ref.py, ONCE -- not once per step: sigma_k(D_d) G_d is
    P sigma_k(c1) sigma_k(s) on the digit's limbs whatever multiple of Q_d ModUp
    added, and one ModDown divides the sum."""
    mod, Bc, Be, rng, s = thh._setup(Lv, K, alpha, bits, 700 + Lv + K)
    m = rng.integers(-(1 << 20), 1 << 20, N)
    c0, c1, me = thh._encrypt(Bc, mod[:Lv], s, m, rng)
    keys = [None if k == 0 else _plain_key(mod, Lv, alpha, s, k) for k in STEPS]
    o0, o1 = rotsum_hybrid_ref(Bc, Be, c0, c1, STEPS, keys, alpha)
    n0, n1 = rotsum_hybrid_ref(Bc, Be, c0, c1, STEPS, keys, alpha, mul=lambda u, v: orc.mul_naive(Be, u, v))
    assert np.array_equal(o0, n0) and np.array_equal(o1, n1)
    got = thh._decrypt(Bc, mod[:Lv], o0, o1, s)
    want = [0] * N
    for k in STEPS:
        r = [int(v) for v in me] if k == 0 else thh._sigma_int(me, k)
        want = [a + b for a, b in zip(want, r)]
    err = max(abs(a - b) for a, b in zip(got, want))
    bound = (K + 1) * (1 + int(np.sum(np.abs(s))))
    print(f"Lv={Lv} K={K} alpha={alpha} bits={bits}: error {err}, ModDown bound {bound}")
    assert err <= bound


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_drawn_keys_stay_within_the_sum_of_the_key_switch_bounds(Lv, K, alpha, bits):
    """With drawn keys every rotating step adds one key-switch error term
    (sigma_k(D_d) has the norm ModUp_d(sigma_k(c1)) is bounded by) and ModDown
    enters once: |NZ| times the key part of thr._bound plus one ModDown part."""
    mod, Bc, Be, rng, s = thh._setup(Lv, K, alpha, bits, 710 + Lv + K)
    m = rng.integers(-(1 << 20), 1 << 20, N)
    c0, c1, me = thh._encrypt(Bc, mod[:Lv], s, m, rng)
    steps = [0, 1, -3, 5]
    keys, emax = [], 0
    for k in steps:
        if k == 0:
            keys.append(None)
            continue
        ka, kb, e = thh._rot_key(Be, mod, Lv, alpha, s, k, rng)
        keys.append((ka, kb))
        emax = max(emax, e)
    o0, o1 = rotsum_hybrid_ref(Bc, Be, c0, c1, steps, keys, alpha)
    got = thh._decrypt(Bc, mod[:Lv], o0, o1, s)
    want = [int(v) for v in me]
    for k in steps[1:]:
        want = [a + b for a, b in zip(want, thh._sigma_int(me, k))]
    err = max(abs(a - b) for a, b in zip(got, want))
    md = (K + 1) * (1 + int(np.sum(np.abs(s))))
    bound = 3 * (thr._bound(mod, Lv, K, alpha, emax, s) - md) + md
    print(f"Lv={Lv} K={K} alpha={alpha} bits={bits}: error {err}, bound {bound}")
    assert err <= bound


@pytest.mark.parametrize("Lv,K,alpha,bits", RINGS)
def test_single_step_decrypts_as_the_rotation_plus_the_ciphertext(Lv, K, alpha, bits):
    """steps = [0, k]: the same decryption as rotate_hybrid_ref(ct, k) + ct,
    within the two calls' bounds -- but not its words (ModUp sees c1 here and
    sigma_k(c1) there)."""
    mod, Bc, Be, rng, s = thh._setup(Lv, K, alpha, bits, 720 + Lv + K)
    m = rng.integers(-(1 << 20), 1 << 20, N)
    c0, c1, _ = thh._encrypt(Bc, mod[:Lv], s, m, rng)
    for k in (1, -3):
        ka, kb, emax = thh._rot_key(Be, mod, Lv, alpha, s, k, rng)
        o0, o1 = rotsum_hybrid_ref(Bc, Be, c0, c1, [0, k], [None, (ka, kb)], alpha)
        r0, r1 = rotate_hybrid_ref(Bc, Be, c0, c1, k, ka, kb, alpha)
        w0, w1 = orc.add(Bc, r0, c0), orc.add(Bc, r1, c1)
        assert not np.array_equal(o0, w0)
        a = thh._decrypt(Bc, mod[:Lv], o0, o1, s)
        b = thh._decrypt(Bc, mod[:Lv], w0, w1, s)
        err = max(abs(x - y) for x, y in zip(a, b))
        bound = 2 * thr._bound(mod, Lv, K, alpha, emax, s)
        print(f"Lv={Lv} K={K} alpha={alpha} bits={bits} k={k}: difference {err}, bound {bound}")
        assert err <= bound


def test_all_zero_steps_give_z_times_the_ciphertext():
    mod, Bc, Be, rng, _ = thh._setup(3, 2, 2, 31, 730)
    c0, c1 = orc.uniform_poly(mod[:3], N, rng), orc.uniform_poly(mod[:3], N, rng)
    o0, o1 = rotsum_hybrid_ref(Bc, Be, c0, c1, [0, 0, 0], [None] * 3, 2)
    q = np.array(mod[:3], dtype=np.uint64)[:, None]
    assert np.array_equal(o0, (3 * c0) % q) and np.array_equal(o1, (3 * c1) % q)
    one0, one1 = rotsum_hybrid_ref(Bc, Be, c0, c1, [0], [None], 2)
    assert np.array_equal(one0, c0) and np.array_equal(one1, c1)


def _exponents(log_n):
    n = 1 << log_n
    return [5, 25, 2 * n - 1, pow(5, 7, 2 * n) * (2 * n - 1) % (2 * n), rotation_exponent(-3, n), 3, 2 * n - 3]


@pytest.mark.parametrize("log_n", [4, 8, 10])
def test_index_function_is_a_bijection_and_maps_aligned_blocks_to_aligned_blocks(log_n):
    """For every block size 2^m an aligned block of positions reads from ONE
    aligned block of the same size: a wave of 64 lanes x 16 bytes gathers from
    one aligned span of its own size (the layout k_rotsum_mac and
    k_automorph_ntt rely on)."""
    n = 1 << log_n
    for g in _exponents(log_n):
        src = ntt_automorphism_source(g, log_n)
        assert sorted(src.tolist()) == list(range(n)), g
        for m in range(log_n + 1):
            blocks = (src >> m).reshape(n >> m, 1 << m)
            assert (blocks == blocks[:, :1]).all(), (g, m)
        assert np.array_equal(ntt_automorphism_source(1, log_n), np.arange(n))


def _host_order(B, log_n):
    """perm[i] = the device position of the oracle's NTT-domain index i, derived
    from the oracle itself: to_ntt(X) holds psi^(2k+1) at the index of
    evaluation point k, and the device stores that point at brv(k)."""
    n = 1 << log_n
    q, psi = int(B.moduli[0]), int(B.psi(0))
    x = np.zeros((B.L, n), dtype=np.uint64)
    x[:, 1] = 1
    vals = orc.to_ntt(B, x)[0]
    where = {pow(psi, 2 * k + 1, q): k for k in range(n)}
    assert len(where) == n
    k = np.array([where[int(v)] for v in vals], dtype=np.int64)
    assert sorted(k.tolist()) == list(range(n))
    from rotsum_ref import _brv
    return _brv(k, log_n)


@pytest.mark.parametrize("log_n", [4, 8, 10])
def test_index_function_is_the_oracles_automorphism_in_the_ntt_domain(log_n):
    n = 1 << log_n
    mod = orc.generate_primes(31, 2, n)
    B = orc.Basis(mod, n)
    perm = _host_order(B, log_n)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    x = orc.uniform_poly(mod, n, np.random.default_rng(740 + log_n))
    xh = orc.to_ntt(B, x)
    for g in _exponents(log_n):
        want = orc.to_ntt(B, orc.automorphism(B, x, g)[0])
        src = ntt_automorphism_source(g, log_n)
        got = xh[:, inv[src[perm]]]  # host i -> device perm[i] -> its source -> host again
        assert np.array_equal(got, want), g
