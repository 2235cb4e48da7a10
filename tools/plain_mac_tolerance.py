#!/usr/bin/env python3
"""The decode error of ``CkksEngine.plain_mac`` measured on the CPU: the
tolerance of tests/test_gpu_plain_mac.py's end-to-end tests.

The evaluator tests' ring -- N = 2^10, 7 ciphertext primes of 30 bits (the
largest below 2^30), scale 2^30, ternary secret of weight N / 2, errors of
width 3.2 -- with 8 terms: 8 encrypted vectors, 8 weight vectors encoded at
2^30 and a bias encoded at 2^60, every value uniform in (-1, 1).  For each seed
the ciphertexts go through tests/plain_mac_ref.py with the rescale (forward
transforms, pointwise sums against the NTT-domain plaintexts, one inverse per
component, rescale_pair); the result is decrypted, decoded at the NOMINAL scale
2^30 and compared with numpy's sum_i w_i a_i + b, so the error includes the
scale drift of q_last != 2^30 that the engine's integer logp ignores.  No
device is touched.  Prints one line per seed and writes the largest error to
profiles/plain_mac_tolerance.txt; the tests allow 4 x that figure.

    python tools/plain_mac_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests"):
    sys.path.insert(0, os.path.join(REPO, p))

import encoder as enc  # noqa: E402
import pyoracle as orc  # noqa: E402
from hybrid_ref import crt_centered  # noqa: E402
from plain_mac_ref import plain_mac_ref  # noqa: E402
from poly_eval_ref import Model  # noqa: E402

N, L, K, ALPHA, LOGP, TERMS = 1024, 7, 2, 2, 30, 8
OUT = os.path.join(REPO, "profiles", "plain_mac_tolerance.txt")


def run(seed):
    q, p = orc.generate_primes(LOGP, L, N), orc.generate_primes(31, K, N)
    m = Model(q, p, N, ALPHA, LOGP, seed)  # (its relinearisation key is not used)
    a, w = m.rng.uniform(-1, 1, (TERMS, N // 2)), m.rng.uniform(-1, 1, (TERMS, N // 2))
    b = m.rng.uniform(-1, 1, N // 2)
    cts = [m.encrypt(v) for v in a]
    x0, x1 = np.stack([c[0] for c in cts]), np.stack([c[1] for c in cts])
    pts = np.stack([orc.to_ntt(m.Bc, orc.from_coeffs(m.Bc, enc.encode_fft(v, N, LOGP))) for v in w])
    bias = orc.to_ntt(m.Bc, orc.from_coeffs(m.Bc, enc.encode_fft(b, N, 2 * LOGP)))
    ct = plain_mac_ref(m.Bc, x0, x1, pts, bias, rescale=True)
    Bl = m.Bc.drop_last(1)
    # decrypt over all L - 1 limbs and lift with the big-integer centred CRT (orc.to_coeffs is exact to 128 bits
    # only; these limbs hold 180), then decode at the nominal scale 2 LOGP - bit_length(q_last) = LOGP
    dec = orc.add(Bl, orc.mul(Bl, ct[1], m.sk[: L - 1]), ct[0])
    coeffs = np.array(crt_centered(dec, q[: L - 1]), dtype=np.int64)
    got = enc.decode_fft(coeffs, N, 2 * LOGP - q[-1].bit_length(), N // 2)
    return float(np.max(np.abs(got - (np.sum(w * a, axis=0) + b))))


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst = 0.0
    for seed in range(n_seeds):
        e = run(seed)
        worst = max(worst, e)
        print(f"seed {seed}: plain_mac of {TERMS} terms + bias {e:.3e}")
    line = (f"plain_mac of {TERMS} terms + bias, N = {N}, {L} x {LOGP}-bit primes, scale 2^{LOGP}: largest decode "
            f"error over {n_seeds} seeds {worst:.3e}; tolerance 4 x = {4 * worst:.3e}")
    print(line)
    with open(OUT, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
