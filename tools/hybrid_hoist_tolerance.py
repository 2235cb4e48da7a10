#!/usr/bin/env python3
"""The decode error of the hoisted hybrid pipelines, measured on the CPU: the
tolerances of tests/test_gpu_hybrid_hoist.py's end-to-end tests.

tools/hybrid_tolerance.py's ring -- N = 2^10, 4 x 31-bit ciphertext primes (the
smallest above 2^30) + 2 special primes (the largest below 2^31), alpha = 2,
scale 2^30, x uniform in (-1, 1) -- with oracle/pyoracle, oracle/encoder.py,
numpy draws and tests/hybrid_hoist_ref.py:

* encode -> encrypt -> rotate_hybrid_hoisted_ref by 1, -3 and 7 -> decrypt ->
  decode against the rolled slots;
* a 16-diagonal band, diagonals at scale 2^30, through bsgs_hybrid_ref with baby
  [0, 1, 2, 3] x giant [0, 4, 8, 12] -> rescale -> decrypt -> decode against M x;
* the same band through the diagonal method (bsgs_hybrid_ref with the sixteen
  steps as babies and the single giant 0), what linear_transform_hybrid runs.

No device is touched.  Prints one line per seed and the largest errors.

    python tools/hybrid_hoist_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", "toy-heaan-ckks_amd", "tools"):
    sys.path.insert(0, os.path.join(REPO, p))

import encoder as enc  # noqa: E402
import pyoracle as orc  # noqa: E402
from hybrid_hoist_ref import bsgs_hybrid_ref, rotate_hybrid_hoisted_ref  # noqa: E402
from hybrid_tolerance import ALPHA, L, LOGP, N, SLOTS, gauss, hybrid_key, ring_moduli, rolled, ternary  # noqa: E402
from rns_ntt import bsgs_diagonal_rows  # noqa: E402

ROT_STEPS = [1, -3, 7]
BABY, GIANT = [0, 1, 2, 3], [0, 4, 8, 12]
DIAGS = list(range(16))


def _setup(seed):
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

    def rot_key(k):
        return hybrid_key(Be, mod, sk_e, orc.rotate_slots(Bc, sk, k)[0], rng)

    return rng, mod, modc, Be, Bc, sk, encrypt, rot_key


def run_rotations(seed):
    rng, mod, modc, Be, Bc, sk, encrypt, rot_key = _setup(seed)
    x = rng.uniform(-1, 1, SLOTS)
    c0, c1 = encrypt(x)
    worst = 0.0
    for k in ROT_STEPS:
        o0, o1 = rotate_hybrid_hoisted_ref(Bc, Be, c0, c1, k, *rot_key(k), ALPHA)
        dec = orc.add(Bc, orc.mul(Bc, o1, sk), o0)
        got = enc.decode_fft(orc.to_coeffs(Bc, dec), N, LOGP, SLOTS)
        worst = max(worst, float(np.max(np.abs(got - rolled(x, k)))))
    return worst


def run_band(seed, baby, giant):
    rng, mod, modc, Be, Bc, sk, encrypt, rot_key = _setup(seed)
    bk = [None if k == 0 else rot_key(k) for k in baby]
    gk = [None if k == 0 else rot_key(k) for k in giant]
    x = rng.uniform(-1, 1, SLOTS)
    M = np.zeros((SLOTS, SLOTS))
    s = np.arange(SLOTS)
    for d in DIAGS:
        M[s, (s + d) % SLOTS] = rng.uniform(-1, 1, SLOTS)
    c0, c1 = encrypt(x)
    rows = bsgs_diagonal_rows(M, baby, giant).reshape(-1, SLOTS)
    diag = np.stack([orc.from_coeffs(Bc, enc.encode_fft(r, N, LOGP)) for r in rows])
    o0, o1 = bsgs_hybrid_ref(Bc, Be, c0, c1, baby, giant, diag, bk, gk, ALPHA)
    r0, r1 = orc.rescale(Bc, o0), orc.rescale(Bc, o1)
    Bd = Bc.drop_last(1)
    dec = orc.add(Bd, orc.mul(Bd, r1, sk[: L - 1]), r0)
    logp = 2 * LOGP - int(modc[-1]).bit_length()
    got = enc.decode_fft(orc.to_coeffs(Bd, dec), N, logp, SLOTS)
    # logp counts the dropped prime as 31 bits; the true scale is 2^60 / q_last
    y = (M @ x) * (2.0 ** (2 * LOGP - logp) / modc[-1])
    return float(np.max(np.abs(got - y)))


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst = [0.0, 0.0, 0.0]
    for seed in range(n_seeds):
        e = (run_rotations(seed), run_band(seed, BABY, GIANT), run_band(seed, DIAGS, [0]))
        worst = [max(w, v) for w, v in zip(worst, e)]
        print(f"seed {seed}: hoisted hybrid rotation {e[0]:.3e}  bsgs hybrid {e[1]:.3e}  diagonal method {e[2]:.3e}")
    for name, w in zip(("hoisted hybrid rotation", "bsgs hybrid 4 x 4", "linear_transform_hybrid, 16 diagonals"), worst):
        print(f"{name}, largest error over {n_seeds} seeds: {w:.3e}; tolerance 4 x = {4 * w:.3e}")


if __name__ == "__main__":
    main()
