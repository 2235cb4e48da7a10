#!/usr/bin/env python3
"""The decode error of ``CkksEngine.dot_ciphertexts_hybrid`` measured on the
CPU: the tolerance of tests/test_gpu_dot_hybrid.py's end-to-end test.

The evaluator tests' ring -- N = 2^10, 7 ciphertext primes of 30 bits (the
largest below 2^30), 2 special primes of 31 bits, alpha = 2, scale 2^30, ternary
secret of weight N / 2, errors of width 3.2 -- with 8 terms whose inputs are
uniform in (-1, 1).  For each seed the 16 ciphertexts go through
tests/dot_hybrid_ref.py (the definition: one key-switch of the summed d2, then
the rescale), the result is decrypted, decoded at the NOMINAL scale 2^30 and
compared with numpy's sum_i a_i b_i; the error therefore includes the scale
drift of q_last != 2^30 that the engine's integer logp ignores.  The same
ciphertexts also go through the loop of hybrid multiplies + rescales + additions
the call replaces, for comparison.  No device is touched.  Prints one line per
seed and the largest errors; the test's tolerance is 4 x the first maximum.

    python tools/dot_tolerance.py [n_seeds]
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
from dot_hybrid_ref import dot_relin_rescale_hybrid_ref  # noqa: E402
from hybrid_ref import crt_centered  # noqa: E402
from hybrid_rescale_ref import mul_relin_rescale_hybrid_ref  # noqa: E402
from poly_eval_ref import Model  # noqa: E402

N, L, K, ALPHA, LOGP, TERMS = 1024, 7, 2, 2, 30, 8


def run(seed):
    q, p = orc.generate_primes(LOGP, L, N), orc.generate_primes(31, K, N)
    m = Model(q, p, N, ALPHA, LOGP, seed)
    a, b = m.rng.uniform(-1, 1, (TERMS, N // 2)), m.rng.uniform(-1, 1, (TERMS, N // 2))
    ca, cb = [m.encrypt(v) for v in a], [m.encrypt(v) for v in b]
    stack = lambda cts, i: np.stack([c[i] for c in cts])  # noqa: E731
    dot = dot_relin_rescale_hybrid_ref(m.Bc, m.Be, stack(ca, 0), stack(ca, 1), stack(cb, 0), stack(cb, 1), m.key_a,
                                       m.key_b, ALPHA)
    Bl = m.Bc.drop_last(1)
    loop = None
    for x, y in zip(ca, cb):
        t = mul_relin_rescale_hybrid_ref(m.Bc, m.Be, x[0], x[1], y[0], y[1], m.key_a, m.key_b, ALPHA)
        loop = t if loop is None else (orc.add(Bl, loop[0], t[0]), orc.add(Bl, loop[1], t[1]))
    want = np.sum(a * b, axis=0)

    def decode(ct):
        """Decrypt over all L - 1 limbs and lift with the big-integer centred CRT
        of tests/hybrid_ref.py (orc.to_coeffs is exact to 128 bits only; these
        limbs hold 180), then decode at the nominal scale."""
        dec = orc.add(Bl, orc.mul(Bl, ct[1], m.sk[: L - 1]), ct[0])
        coeffs = np.array(crt_centered(dec, q[: L - 1]), dtype=np.int64)
        return enc.decode_fft(coeffs, N, LOGP, N // 2)

    return tuple(float(np.max(np.abs(decode(ct) - want))) for ct in (dot, loop))


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst = [0.0, 0.0]
    for seed in range(n_seeds):
        e = run(seed)
        worst = [max(w, v) for w, v in zip(worst, e)]
        print(f"seed {seed}: dot of {TERMS} terms {e[0]:.3e}  looped multiplies {e[1]:.3e}")
    print(f"dot of {TERMS} terms, largest error over {n_seeds} seeds: {worst[0]:.3e}; tolerance 4 x = "
          f"{4 * worst[0]:.3e}")
    print(f"looped multiplies, largest error over {n_seeds} seeds: {worst[1]:.3e}")


if __name__ == "__main__":
    main()
