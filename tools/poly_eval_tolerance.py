#!/usr/bin/env python3
"""The decode error of ``CkksEngine.evaluate_polynomial_hybrid`` measured on the
CPU: the tolerance of tests/test_gpu_poly_eval.py and tests/test_poly_eval_ref.py.

The tests' ring -- N = 2^10, 7 ciphertext primes of 30 bits (the largest below
2^30), 2 special primes of 31 bits, alpha = 2, scale 2^30, ternary secret of
weight N / 2, errors of width 3.2 -- with inputs and coefficients uniform in
(-1, 1).  For each seed and each (degree, basis) of the tests the plan of
rns_ntt.poly_eval_plan runs on tests/poly_eval_ref.py (oracle/pyoracle,
tests/hybrid_ref.py with restrict_key of one full-level key,
tests/lincomb_ref.py), the result is decrypted, decoded at the NOMINAL scale
2^30 and compared with numpy.polyval / chebval of the plain inputs.  The error
therefore includes the scale drift of q_last != 2^30 that the engine's integer
logp ignores, besides the rounding of the weights and the key-switch noise.  No
device is touched.  Prints one line per seed and case and the largest error per
case; the tests' tolerance is 4 x that maximum.

    python tools/poly_eval_tolerance.py [n_seeds]
"""
from __future__ import annotations

import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "tests", os.path.join("toy-heaan-ckks_amd", "rns_ntt")):
    sys.path.insert(0, os.path.join(REPO, p))

import pyoracle as orc  # noqa: E402
from poly_eval import poly_eval_plan  # noqa: E402  (the pure host module: no library needed)
from poly_eval_ref import Model, plain_value  # noqa: E402

N, L, K, ALPHA, LOGP = 1024, 7, 2, 2, 30
CASES = [(7, "monomial"), (7, "chebyshev"), (15, "monomial"), (15, "chebyshev")]


def ring_moduli():
    return orc.generate_primes(LOGP, L, N), orc.generate_primes(31, K, N)


def run(seed, degree, basis):
    q, p = ring_moduli()
    model = Model(q, p, N, ALPHA, LOGP, seed)
    x = model.rng.uniform(-1, 1, N // 2)
    coeffs = model.rng.uniform(-1, 1, degree + 1)
    plan = poly_eval_plan(coeffs, basis, LOGP)
    got = model.decode(model.runner.run(plan, model.encrypt(x)))
    return float(np.max(np.abs(got - plain_value(coeffs, basis, x))))


def main():
    n_seeds = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    worst = {c: 0.0 for c in CASES}
    for seed in range(n_seeds):
        for c in CASES:
            e = run(seed, *c)
            worst[c] = max(worst[c], e)
            print(f"seed {seed}: degree {c[0]:2d} {c[1]:9s} decode error {e:.3e}")
    for c in CASES:
        print(f"degree {c[0]:2d} {c[1]:9s}: largest error over {n_seeds} seeds {worst[c]:.3e}; "
              f"tolerance 4 x = {4 * worst[c]:.3e}")


if __name__ == "__main__":
    main()
