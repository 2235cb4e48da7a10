#!/usr/bin/env python3
"""The decode error of the hybrid key-switch's end-to-end pipelines, measured
on the CPU: the tolerances of tests/test_gpu_hybrid.py's end-to-end test.

At N = 2^10, 4 x 31-bit ciphertext primes (the smallest above 2^30, so that a
rescale keeps the scale) + 2 special primes (the largest below 2^31, so that
P >= alpha max Q_d), alpha = 2, ciphertext scale 2^30 (one prime per level),
x and y uniform in (-1, 1), with oracle/pyoracle, oracle/encoder.py, numpy draws and tests/hybrid_ref.py:

* encode -> encrypt -> rotate_hybrid_ref by 1 and by -3 -> decrypt -> decode
  against the rolled slots;
* encrypt x and y -> mul_relin_hybrid_ref -> rescale -> decrypt -> decode
  against x * y;
* the gadget rotation (orc.rotate_ciphertext) of the same ciphertext at the same
  scale, to show what the one-limb gadget's noise does to a 2^30 message.

No device is touched.  Prints one line per seed and the largest errors.

    python tools/hybrid_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "tools"):
    sys.path.insert(0, os.path.join(REPO, p))

import encoder as enc  # noqa: E402
import pyoracle as orc  # noqa: E402
from hybrid_ref import hybrid_key_plain, mul_relin_hybrid_ref, n_digits, rotate_hybrid_ref  # noqa: E402

N, SLOTS, L, K, ALPHA = 1024, 512, 4, 2, 2
LOGP = 30
SIGMA, HW = 3.2, N // 2
ROT_STEPS = [1, -3]


def _is_prime(v):
    if v < 2 or v % 2 == 0:
        return v == 2
    d, r = v - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if a % v == 0:
            continue
        x = pow(a, d, v)
        if x in (1, v - 1):
            continue
        for _ in range(r - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


def ring_moduli():
    """(q_0..q_{L-1}, p_0..p_{K-1}): the L smallest NTT-friendly primes above
    2^30 and the K largest below 2^31."""
    q, c = [], (1 << 30) + 1
    while len(q) < L:
        if _is_prime(c):
            q.append(c)
        c += 2 * N
    return q + orc.generate_primes(31, K, N)


def ternary(rng):
    c = np.zeros(N, dtype=np.int64)
    idx = rng.choice(N, size=HW, replace=False)
    c[idx] = rng.choice(np.array([-1, 1], dtype=np.int64), size=HW)
    return c


def gauss(Bo, rng):
    return orc.from_coeffs(Bo, np.rint(rng.normal(0.0, SIGMA, size=N)).astype(np.int64))


def rolled(x, k):
    r = np.roll(x, -abs(int(k)))
    return np.conj(r) if k < 0 else r


def hybrid_key(Be, mod, sk_e, target, rng):
    """b_d = -(a_d s) + e_d + G_d over E for the target's residues over C."""
    G = hybrid_key_plain(mod, L, ALPHA, target)
    ka = orc.uniform_poly(mod, N, rng, batch=n_digits(L, ALPHA))
    kb = np.zeros_like(ka)
    for d in range(ka.shape[0]):
        kb[d] = orc.add(Be, orc.add(Be, orc.neg(Be, orc.mul(Be, ka[d], sk_e)), gauss(Be, rng)), G[d])
    return ka, kb


def gadget_key(Bc, modc, sk, target, rng):
    ka = orc.uniform_poly(modc, N, rng, batch=L)
    kb = np.zeros_like(ka)
    for i in range(L):
        plain = np.zeros((L, N), dtype=np.uint64)
        plain[i] = target[i]
        kb[i] = orc.add(Bc, orc.add(Bc, orc.neg(Bc, orc.mul(Bc, ka[i], sk)), gauss(Bc, rng)), plain)
    return ka, kb


def run(seed):
    rng = np.random.default_rng(seed)
    mod = ring_moduli()
    modc = mod[:L]
    Be, Bc = orc.Basis(mod, N), orc.Basis(modc, N)
    s = ternary(rng)
    sk, sk_e = orc.from_coeffs(Bc, s), orc.from_coeffs(Be, s)
    a = orc.uniform_poly(modc, N, rng)
    pk_b = orc.add(Bc, orc.neg(Bc, orc.mul(Bc, a, sk)), gauss(Bc, rng))

    def encrypt(v):
        m = orc.from_coeffs(Bc, enc.encode_fft(v, N, LOGP))
        u = orc.from_coeffs(Bc, ternary(rng))
        c0 = orc.add(Bc, orc.add(Bc, orc.mul(Bc, pk_b, u), gauss(Bc, rng)), m)
        return c0, orc.add(Bc, orc.mul(Bc, a, u), gauss(Bc, rng))

    x, y = rng.uniform(-1, 1, SLOTS), rng.uniform(-1, 1, SLOTS)
    cx, cy = encrypt(x), encrypt(y)
    e_rot = e_gad = 0.0
    for k in ROT_STEPS:
        target, _ = orc.rotate_slots(Bc, sk, k)
        o0, o1 = rotate_hybrid_ref(Bc, Be, cx[0], cx[1], k, *hybrid_key(Be, mod, sk_e, target, rng), ALPHA)
        g0, g1 = orc.rotate_ciphertext(Bc, cx[0], cx[1], k, *gadget_key(Bc, modc, sk, target, rng))
        for name, (p0, p1) in (("h", (o0, o1)), ("g", (g0, g1))):
            dec = orc.add(Bc, orc.mul(Bc, p1, sk), p0)
            got = enc.decode_fft(orc.to_coeffs(Bc, dec), N, LOGP, SLOTS)
            err = float(np.max(np.abs(got - rolled(x, k))))
            if name == "h":
                e_rot = max(e_rot, err)
            else:
                e_gad = max(e_gad, err)
    rlk = hybrid_key(Be, mod, sk_e, orc.mul(Bc, sk, sk), rng)
    o0, o1 = mul_relin_hybrid_ref(Bc, Be, cx[0], cx[1], cy[0], cy[1], *rlk, ALPHA)
    r0, r1 = orc.rescale(Bc, o0), orc.rescale(Bc, o1)
    Bd = Bc.drop_last(1)
    dec = orc.add(Bd, orc.mul(Bd, r1, sk[: L - 1]), r0)
    logp = 2 * LOGP - int(modc[-1]).bit_length()
    got = enc.decode_fft(orc.to_coeffs(Bd, dec), N, logp, SLOTS)
    # the ciphertext's logp counts the dropped prime as 31 bits; the true scale
    # after the rescale is 2^60 / q_last, which the expected slots carry
    e_mul = float(np.max(np.abs(got - x * y * (2.0 ** (2 * LOGP - logp) / modc[-1]))))
    return e_rot, e_mul, e_gad


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst = [0.0, 0.0, 0.0]
    for seed in range(n_seeds):
        e = run(seed)
        worst = [max(w, v) for w, v in zip(worst, e)]
        print(f"seed {seed}: hybrid rotation {e[0]:.3e}  hybrid multiply + rescale {e[1]:.3e}  "
              f"gadget rotation at the same scale {e[2]:.3e}")
    print(f"hybrid rotation, largest error over {n_seeds} seeds: {worst[0]:.3e}; tolerance 4 x = {4 * worst[0]:.3e}")
    print(f"hybrid multiply + rescale, largest error over {n_seeds} seeds: {worst[1]:.3e}; "
          f"tolerance 4 x = {4 * worst[1]:.3e}")
    print(f"gadget rotation at scale 2^{LOGP}, largest error over {n_seeds} seeds: {worst[2]:.3e}")


if __name__ == "__main__":
    main()
