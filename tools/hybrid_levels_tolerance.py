#!/usr/bin/env python3
"""The decode error of a three-level hybrid circuit that uses ONE full-level
relinearisation key and ONE full-level rotation key at every level, measured on
the CPU: the tolerance of tests/test_gpu_hybrid_levels.py's end-to-end test.

tools/hybrid_tolerance.py's ring (N = 2^10, 4 x 31-bit ciphertext primes just
above 2^30, 2 special primes, alpha = 2, scale 2^30, x, y, w uniform in
(-1, 1)) and its sampling, with oracle/pyoracle, oracle/encoder.py and
tests/hybrid_ref.py:

    rot_1( ((x * y) rescaled * w) rescaled )

* level 4: mul_relin_hybrid_ref with the full key, rescale;
* level 3: w's ciphertext with its last limb dropped, mul_relin_hybrid_ref with
  restrict_key(key, 4, alpha, 3), rescale;
* level 2: rotate_hybrid_ref by 1 with restrict_key(rotation key, 4, alpha, 2);
* decrypt, decode against roll(x y w, -1) at the true scale 2^90 / (q_3 q_2).

The level keys are restrictions of the full keys: the words a key level view
reads (rnt_key_level_view).  No device is touched.  Prints one line per seed
and the largest error.

    python tools/hybrid_levels_tolerance.py [n_seeds]
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
from hybrid_ref import mul_relin_hybrid_ref, restrict_key, rotate_hybrid_ref  # noqa: E402
from hybrid_tolerance import ALPHA, K, L, LOGP, N, SLOTS, gauss, hybrid_key, ring_moduli, ternary  # noqa: E402

STEP = 1


def run(seed):
    rng = np.random.default_rng(seed)
    mod = ring_moduli()
    q, p = mod[:L], mod[L:]
    Be, Bc = orc.Basis(mod, N), orc.Basis(q, N)
    s = ternary(rng)
    sk, sk_e = orc.from_coeffs(Bc, s), orc.from_coeffs(Be, s)
    a = orc.uniform_poly(q, N, rng)
    pk_b = orc.add(Bc, orc.neg(Bc, orc.mul(Bc, a, sk)), gauss(Bc, rng))

    def encrypt(v):
        m = orc.from_coeffs(Bc, enc.encode_fft(v, N, LOGP))
        u = orc.from_coeffs(Bc, ternary(rng))
        c0 = orc.add(Bc, orc.add(Bc, orc.mul(Bc, pk_b, u), gauss(Bc, rng)), m)
        return c0, orc.add(Bc, orc.mul(Bc, a, u), gauss(Bc, rng))

    x, y, w = (rng.uniform(-1, 1, SLOTS) for _ in range(3))
    cx, cy, cw = encrypt(x), encrypt(y), encrypt(w)
    rlk = hybrid_key(Be, mod, sk_e, orc.mul(Bc, sk, sk), rng)
    rotk = hybrid_key(Be, mod, sk_e, orc.rotate_slots(Bc, sk, STEP)[0], rng)
    # level 4 -> 3
    o0, o1 = mul_relin_hybrid_ref(Bc, Be, cx[0], cx[1], cy[0], cy[1], *rlk, ALPHA)
    c0, c1 = orc.rescale(Bc, o0), orc.rescale(Bc, o1)
    # level 3 -> 2
    B3, E3 = orc.Basis(q[:3], N), orc.Basis(q[:3] + p, N)
    k3 = [restrict_key(h, L, ALPHA, 3) for h in rlk]
    o0, o1 = mul_relin_hybrid_ref(B3, E3, c0, c1, np.ascontiguousarray(cw[0][:3]), np.ascontiguousarray(cw[1][:3]),
                                  *k3, ALPHA)
    c0, c1 = orc.rescale(B3, o0), orc.rescale(B3, o1)
    # level 2
    B2, E2 = orc.Basis(q[:2], N), orc.Basis(q[:2] + p, N)
    k2 = [restrict_key(h, L, ALPHA, 2) for h in rotk]
    c0, c1 = rotate_hybrid_ref(B2, E2, c0, c1, STEP, *k2, ALPHA)
    dec = orc.add(B2, orc.mul(B2, c1, sk[:2]), c0)
    got = enc.decode_fft(orc.to_coeffs(B2, dec), N, LOGP, SLOTS)
    want = np.roll(x * y * w, -STEP) * (2.0 ** (2 * LOGP) / (q[3] * q[2]))
    return float(np.max(np.abs(got - want)))


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    assert K == 2 and L == 4
    worst = 0.0
    for seed in range(n_seeds):
        e = run(seed)
        worst = max(worst, e)
        print(f"seed {seed}: rot_1(((x y) rescaled w) rescaled) decode error {e:.3e}")
    print(f"largest error over {n_seeds} seeds: {worst:.3e}; tolerance 4 x = {4 * worst:.3e}")


if __name__ == "__main__":
    main()
